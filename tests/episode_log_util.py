"""TEST HELPER: the episode log (csrc/env_episode_log.hpp) restated in numpy from the lane's rule alone, driven by
recorded (reward, done, goals-reached counter) sequences; the fp32 running sum is taken in step order.

    a = fl32(acc + r);  t = age + 1
    done == 0:  acc = a; age = t
    done != 0:  k = TERMINATED if reached != seen else TRUNCATED;  seen = reached;  c = count
                c < E: ret[c] = a; len[c] = t; kind[c] = k; count = c + 1; c + 1 == E: full += 1
                acc = 0; age = 0
"""
import numpy as np

TERMINATED, TRUNCATED = 1, 2
SUMS = ("n_records", "sum_return", "sum_return_sq", "sum_length", "n_terminated", "n_truncated", "n_complete")


class EpisodeLogModel:
    def __init__(self, n, capacity, reached=None):
        self.n, self.E = int(n), int(capacity)
        self.acc = np.zeros(n, np.float32)
        self.age = np.zeros(n, np.uint32)
        self.count = np.zeros(n, np.uint32)
        self.reached = np.zeros(n, np.uint32) if reached is None else np.array(reached, np.uint32)      # the env's own counter
        self.seen = self.reached.copy()
        self.ret = np.zeros((self.E, n), np.float32)
        self.len = np.zeros((self.E, n), np.uint32)
        self.kind = np.zeros((self.E, n), np.uint32)
        self.full = 0

    def step(self, reward, done, reached, lo=0, hi=None):
        """one env step over the envs [lo, hi): reward [hi - lo] float32, done flags, the counters as the step left them (uint32)"""
        hi = self.n if hi is None else hi
        sl = slice(lo, hi)
        reward = np.asarray(reward, np.float32)
        done = np.asarray(done) != 0
        reached = np.asarray(reached, np.uint32)
        a = (self.acc[sl] + reward).astype(np.float32)
        t = self.age[sl] + np.uint32(1)
        kind = np.where(reached != self.seen[sl], TERMINATED, TRUNCATED).astype(np.uint32)
        self.seen[sl] = np.where(done, reached, self.seen[sl])
        c = self.count[sl].copy()
        write = done & (c < self.E)
        idx = lo + np.nonzero(write)[0]
        self.ret[c[write], idx] = a[write]
        self.len[c[write], idx] = t[write]
        self.kind[c[write], idx] = kind[write]
        self.count[sl] = np.where(write, c + np.uint32(1), c)
        self.full += int((write & (c + 1 == self.E)).sum())
        self.acc[sl] = np.where(done, np.float32(0), a)
        self.age[sl] = np.where(done, np.uint32(0), t)

    def step_outcome(self, reward, done, terminated, lo=0, hi=None):
        """the same from what an env reports: the counter moves where an episode ended at its goal"""
        hi = self.n if hi is None else hi
        self.reached[lo:hi] += ((np.asarray(done) != 0) & np.asarray(terminated, bool)).astype(np.uint32)
        self.step(reward, done, self.reached[lo:hi], lo, hi)

    def reset(self):
        """a reset: the episode under way is dropped; `seen` follows the counters (which a reset does not move)"""
        self.acc[:] = 0
        self.age[:] = 0
        self.seen[:] = self.reached

    def counters_cleared(self):
        """stats(reset=True): the counters and `seen` go to zero together"""
        self.reached[:] = 0
        self.seen[:] = 0

    def clear(self):
        self.count[:] = 0
        self.full = 0
        self.reset()

    def log(self):
        """as RoboyVecEnv.episode_log() returns it"""
        live = np.arange(self.E)[None, :] < self.count.astype(np.int64)[:, None]
        return {"count": self.count.astype(np.int64), "return": np.where(live, self.ret.T, np.float32(0)),
                "length": np.where(live, self.len.T.astype(np.int64), 0), "kind": np.where(live, self.kind.T.astype(np.int64), 0)}


def same_log(a, b):
    return all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()
               for k in ("count", "return", "length", "kind"))


def summary_np(log, first_k):
    """the eight sums over the records k < min(count, first_k), in float64 (numpy's order), and the sum of |return| and return^2 terms
    the tolerances are relative to"""
    count, k = log["count"], int(first_k)
    E = log["return"].shape[1]
    live = np.arange(E)[None, :] < np.minimum(count, k)[:, None]
    r = log["return"].astype(np.float64)[live]
    sums = {"n_records": float(live.sum()), "sum_return": float(r.sum()), "sum_return_sq": float((r * r).sum()),
            "sum_length": float(log["length"][live].sum()), "n_terminated": float((log["kind"][live] == TERMINATED).sum()),
            "n_truncated": float((log["kind"][live] == TRUNCATED).sum()), "n_complete": float((count >= k).sum())}
    return sums, float(np.abs(r).sum()), float((r * r).sum())


def figures_np(sums, num_envs):
    """mean, std, rates from the sums, written out again"""
    n = sums["n_records"]
    mean = sums["sum_return"] / n
    return {"mean_return": mean, "std_return": np.sqrt(max(sums["sum_return_sq"] / n - mean * mean, 0.0)), "mean_length": sums["sum_length"] / n,
            "success_rate": sums["n_terminated"] / n, "truncated_rate": sums["n_truncated"] / n, "complete": sums["n_complete"] == num_envs}
