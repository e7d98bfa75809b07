"""TEST INFRASTRUCTURE - the multi-rank PPO update held to one process and to float64 (tests/test_multi_rank_update_cpu.py,
tests/test_multi_rank_update_gpu.py).

What is here: synthetic rollouts in which every branch of the two clipped losses occurs and whose approx_kl is a chosen number; a stub
env (``PPO.update(roll, sample_orders=...)`` never touches the env); the entry point of a rank (gloo on 127.0.0.1, a list of scenarios,
one result file per scenario); the launcher of the ranks (fresh child processes, each under its own time limit); the float64 statement
of ONE optimiser step of W ranks (oracle/policy_ref.py: adv_stats64 and ppo_grad64 per rank, the sum over the ranks, clip_adam64 with
grad_scale = 1 / W at the rate tests/ppo_diag_ref.adapt_lr gives on the mean KL); and the assertions both test files share.

Two kinds of scenario.  "same": every rank is fed the rollouts and sample orders a single process was fed - the all-reduced vector is
g + g, times 0.5 it is g, so two ranks must reproduce the single process bit for bit.  "own": every rank builds its own rollout (from
the current parameters, so that its KL is the chosen one) and its own order, one optimiser step per update; the parent restates each
step in float64 from the state the device held in front of it, so the bounds are a step's and do not compound."""
import datetime
import math
import os
import socket
import subprocess
import sys

import numpy as np
import torch

from gym_roboy_amd._policy_native import PARAM_ORDER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, ACT = 4, 8
CLIPRANGE, VF_COEF, ENT_COEF, LR = 0.2, 0.5, 0.1, 2.5e-4
BETAS, ADAM_EPS = (0.9, 0.999), 1e-5
SCHED = dict(desired_kl=0.01, lr_factor=1.5, lr_min=1e-5, lr_max=1e-2)
CHILD_LIMIT = 240          # seconds per child (tests/test_obs_norm_gpu.py's limit for the same kind of work)
NEAR, FAR_LO, FAR_HI = 0.03, 0.27, 0.33     # |logp - logp_old| of the samples inside / outside the clip range (ratios 1.03; 1.31 .. 1.39)

# per-rank KLs of the three updates of an "own" scenario and the decision of (the mean, rank 0's own, the sum) under desired_kl = 0.01:
# the three decisions part in the first update; in the second the mean raises the rate, in the third it cuts it where rank 0 keeps it
KLS = {2: [[0.002, 0.022], [0.001, 0.003], [0.012, 0.040]],
       3: [[0.002, 0.004, 0.030], [0.001, 0.003, 0.002], [0.012, 0.030, 0.040]]}
DECISIONS = {2: [("keep", "rise", "cut"), ("rise", "rise", "rise"), ("cut", "keep", "cut")],
             3: [("keep", "rise", "cut"), ("rise", "rise", "keep"), ("cut", "keep", "cut")]}


class StubEnv:
    """what PPO's constructor reads of an env: the two spaces, num_envs, critic_obs_dim"""

    def __init__(self, obs_dim, act_dim, num_envs, critic_obs_dim=None):
        from gym_roboy_amd._gymcompat import spaces
        self.observation_space = spaces.Box(low=-1, high=1, shape=(obs_dim,), dtype="float32")
        self.action_space = spaces.Box(low=-1, high=1, shape=(act_dim,), dtype="float32")
        self.num_envs, self.critic_obs_dim = num_envs, critic_obs_dim


class Rows:
    """what oracle/policy_ref.ppo_grad64 and tests/ppo_diag_ref.diag64 need of a policy, over rows [obs | cobs] that were normalised
    already (tests/test_policy_asym_gpu.py: _Split)"""

    def __init__(self, policy, da, dc):
        self.p, self.da, self.dc = policy, da, dc

    def parameters(self):
        return self.p.parameters()

    def dist(self, rows):
        return self.p.dist(rows[:, :self.da])

    def value(self, rows):
        return self.p.value(rows[:, self.da:] if self.dc is not None else rows)


def initial_policy_state(da, dc, seed):
    """MlpPolicy's state_dict - not the near-zero last layer of a fresh policy: every weight counts (tests/test_policy_gpu.py)"""
    from gym_roboy_amd.ppo import MlpPolicy
    torch.manual_seed(seed)
    p = MlpPolicy(da, ACT, critic_obs_dim=dc)
    with torch.no_grad():
        for q in p.parameters():
            q.add_(0.3 * torch.randn_like(q))
    return {k: v.clone() for k, v in p.state_dict().items()}


def scenario(name, kind, da, dc=None, n_envs=96, nminibatches=4, noptepochs=2, updates=2, fused=True, lr_schedule=None,
             normalize_obs=False, kls=None, max_grad_norm=0.5, seed=0):
    """kind "same" / "own" (the module's docstring).  kls[update][rank]: the approx_kl every rollout is built to."""
    return dict(name=name, kind=kind, da=da, dc=dc, n_envs=n_envs, nminibatches=nminibatches, noptepochs=noptepochs, updates=updates,
                fused=fused, lr_schedule=lr_schedule, normalize_obs=normalize_obs, kls=kls, max_grad_norm=max_grad_norm, seed=seed,
                policy_state=initial_policy_state(da, dc, 11 + da + (dc or 0)), rolls=None, orders=None)


def policy64(params, da, dc):
    """a float64 MlpPolicy with the parameters {layout name: tensor} of a snapshot"""
    from gym_roboy_amd.ppo import MlpPolicy, _flat_names
    p = MlpPolicy(da, ACT, critic_obs_dim=dc).double()
    with torch.no_grad():
        for name, q in _flat_names(p).items():
            q.copy_(params[name].double())
    return p


def net_rows(rows32, norm):
    """What the networks see of raw float32 rows under a snapshot's statistics, as float64: ObsNorm.apply's float32 operand (the
    kernels compute the same bits: tests/test_obs_norm_gpu.py)."""
    if norm is None:
        return rows32.double()
    n = norm["norm"]
    return ((rows32 - n[0]) * n[1]).clamp(-norm["clip"], norm["clip"]).double()


def build_rollout(pol64, da, dc, n_envs, seed, kl, norm_a=None, norm_c=None, adv_shift=0.0, adv_scale=1.0):
    """A [T, n_envs, ...] float32 rollout built as tests/test_policy_asym_gpu.py's _case builds its minibatch - actions around the policy's
    mean, old values near and far, returns a unit away - with the old log-probabilities sized for approx_kl = kl: |x| = NEAR for most
    samples, |x| in [FAR_LO, FAR_HI] (ratios outside 1 -+ 0.2 on both sides) for as many as the KL has room for, those then scaled so
    that mean 0.5 x^2 is kl.  Every sample is clear of the clip boundaries.  Critic rows come from another distribution than the
    observation (uniform on [1, 3] against [-2, 2])."""
    g = torch.Generator().manual_seed(seed)
    n = T * n_envs
    obs = (torch.rand(n, da, generator=g, dtype=torch.float64) * 4 - 2).float()
    cobs = (torch.rand(n, dc, generator=g, dtype=torch.float64) * 2 + 1).float() if dc is not None else None
    x, cx = net_rows(obs, norm_a), (net_rows(cobs, norm_c) if dc is not None else None)
    with torch.no_grad():
        d = pol64.dist(x)
        act = (d.mean + d.stddev * torch.randn(n, ACT, generator=g, dtype=torch.float64)).float()
        logp = d.log_prob(act.double()).sum(-1)
        v = pol64.value(cx if dc is not None else x)
    half_near, half_far = 0.5 * NEAR ** 2, 0.5 * (FAR_LO ** 2 + FAR_LO * FAR_HI + FAR_HI ** 2) / 3.0
    n_far = min(max(int(math.floor((kl - half_near) / (half_far - half_near) * n)), 1), n - 1)
    far = torch.randperm(n, generator=g)[:n_far]
    mag = torch.full((n,), NEAR, dtype=torch.float64)
    mag[far] = FAR_LO + (FAR_HI - FAR_LO) * torch.rand(n_far, generator=g, dtype=torch.float64)
    mag[far] *= math.sqrt((kl * n - (n - n_far) * half_near) / (0.5 * mag[far] ** 2).sum().item())
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    logp_old = (logp - sign * mag).float()
    adv = (torch.randn(n, generator=g, dtype=torch.float64) * adv_scale + adv_shift).float()
    val_old = v + (torch.rand(n, generator=g, dtype=torch.float64) - 0.5) * 6 * CLIPRANGE
    val_old = torch.where(((v - val_old).abs() - CLIPRANGE).abs() < 1e-3, val_old + 0.01, val_old).float()
    ret = (v + torch.randn(n, generator=g, dtype=torch.float64)).float()
    # the float32 rollout, judged in float64: the KL is the chosen one and no sample sits on a clip boundary
    xs = logp - logp_old.double()
    ratio = xs.exp()
    assert abs((0.5 * xs * xs).mean().item() / kl - 1.0) < 1e-3, ((0.5 * xs * xs).mean().item(), kl)
    assert torch.minimum((ratio - (1 - CLIPRANGE)).abs(), (ratio - (1 + CLIPRANGE)).abs()).min().item() > 1e-2
    assert (((v - val_old.double()).abs() - CLIPRANGE).abs() > 1e-4).all()
    roll = {"obs": obs, "act": act, "logp": logp_old, "val": val_old, "adv": adv, "ret": ret}
    if dc is not None:
        roll["cobs"] = cobs
    return {k: t.reshape(T, n_envs, *t.shape[1:]).contiguous() for k, t in roll.items()}


def make_agent(spec, device, dist=None):
    from gym_roboy_amd.ppo import PPO, MlpPolicy
    policy = MlpPolicy(spec["da"], ACT, critic_obs_dim=spec["dc"])
    policy.load_state_dict(spec["policy_state"])
    fused = bool(spec["fused"]) and str(device) != "cpu"
    return PPO(StubEnv(spec["da"], ACT, spec["n_envs"], spec["dc"]), policy=policy, n_steps=T, nminibatches=spec["nminibatches"],
               noptepochs=spec["noptepochs"], learning_rate=LR, cliprange=CLIPRANGE, ent_coef=ENT_COEF, vf_coef=VF_COEF,
               max_grad_norm=spec["max_grad_norm"], device=device, dist=dist, seed=3, fused_policy=fused, fused_update=fused,
               normalize_obs=spec["normalize_obs"], asymmetric_critic=spec["dc"] is not None, lr_schedule=spec["lr_schedule"], **SCHED)


def snapshot(agent):
    """parameters, both Adam moments ({layout name: tensor} on the host), the step count, the rate and the observation statistics"""
    from gym_roboy_amd.ppo import _flat_names
    names = _flat_names(agent.policy)
    s = {"params": {k: p.detach().cpu().clone() for k, p in names.items()}}
    if agent._fgrad is not None:
        fa, lay = agent._fadam, agent._fgrad._layout
        cut = lambda flat: {k: flat[lay[k][0]:lay[k][0] + p.numel()].view(p.shape).cpu().clone() for k, p in names.items()}
        s["m"], s["v"], s["t"] = cut(fa.m), cut(fa.v), int(fa.t)
    else:
        st = {k: agent.opt.state.get(p) for k, p in names.items()}
        for key, field in (("m", "exp_avg"), ("v", "exp_avg_sq")):
            s[key] = {k: (st[k][field].detach().cpu().clone() if st[k] else torch.zeros_like(p, device="cpu")) for k, p in names.items()}
        s["t"] = max([int(x["step"]) for x in st.values() if x] or [0])
    s["lr"] = float(agent.learning_rate)
    for key, n in (("obs_norm", agent.obs_norm), ("cobs_norm", agent.cobs_norm)):
        if n is not None:
            s[key] = {"state": n.state.cpu().clone(), "norm": n.norm.cpu().clone(), "clip": float(n.clip)}
    return s


def run_scenario(spec, device, dist=None, rank=0):
    """The updates of one scenario on one rank (or in a single process: dist None).  Fed ``spec["rolls"]`` / ``spec["orders"]`` where they
    are given; otherwise every update's rollout is built from the parameters and statistics the agent holds, with this rank's KL."""
    agent = make_agent(spec, device, dist)
    if spec["lr_schedule"] is not None:
        agent.lr_history = []
    n = T * spec["n_envs"]
    out = {"fused": agent._fgrad is not None, "updates": []}
    for k in range(spec["updates"]):
        pre = snapshot(agent)
        if spec["rolls"] is not None:
            roll, orders = spec["rolls"][k], spec["orders"][k]
        else:
            seed = 100000 * spec["seed"] + 1000 * k + rank
            pol = policy64(pre["params"], spec["da"], spec["dc"])
            roll = build_rollout(pol, spec["da"], spec["dc"], spec["n_envs"], seed, spec["kls"][k][rank], pre.get("obs_norm"),
                                 pre.get("cobs_norm"), adv_shift=0.5 * rank, adv_scale=1.0 + rank)
            g = torch.Generator().manual_seed(seed + 500)
            orders = [torch.randperm(n, generator=g) for _ in range(spec["noptepochs"])]
        seen = len(agent.lr_history or [])
        stats = agent.update({key: t.to(device) for key, t in roll.items()}, sample_orders=[o.to(device) for o in orders])
        if str(device) != "cpu":
            torch.cuda.synchronize()
        hist = [(float(a), float(b)) for a, b in (agent.lr_history or [])[seen:]]
        out["updates"].append({"pre": pre, "post": snapshot(agent), "roll": roll, "orders": orders,
                               "stats": {key: float(val) for key, val in stats.items()}, "lr_history": hist})
    return out


def run_real_envs(spec, dist, rank):
    """The collect side on a rank's own shard of real envs: two rounds of collect() and update() under every statistic PPO keeps, and
    the rows of every rollout it ran - the priming one too."""
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    n = spec["n_envs"]
    env = RoboyVecEnv(MsjRobot(), n, seed=0, env_id_offset=n * rank, tendon_obs=("length", "force"), critic_obs=("state", "age"),
                      report_truncation=True, max_episode_length=3)
    agent = PPO(env, n_steps=T, seed=5, dist=dist, reward_scale=spec["reward_scale"], fused_policy=True, fused_update=True,
                asymmetric_critic=True, normalize_obs=True, normalize_reward=True, bootstrap_timeouts=True, use_graphs=True)
    log, inner = [], agent._collect_rollout

    def recorded():
        roll = inner()
        torch.cuda.synchronize()
        rec = {k: roll[k].cpu().clone() for k in ("obs", "cobs", "done", "trunc")}
        rec["rew_raw"] = agent._rew_raw.cpu().clone()
        log.append(rec)
        return roll

    agent._collect_rollout = recorded
    for _ in range(2):
        agent.update(agent.collect())
    torch.cuda.synchronize()
    out = {"rollouts": log, "params": [p.detach().cpu().clone() for p in agent.policy.parameters()], "gamma": float(agent.gamma),
           "graph": agent._rollout_graph is not None, "num_timesteps": int(agent.num_timesteps)}
    for key, s in (("obs_norm", agent.obs_norm), ("cobs_norm", agent.cobs_norm), ("reward_norm", agent.reward_norm)):
        out[key] = {"state": s.state.cpu().clone(), "norm": s.norm.cpu().clone()}
    env.close()
    return out


def rank_main(rank, world, port, out_dir):
    """A rank: the process group over gloo on 127.0.0.1, the scenarios of ``spec.pt``, one result file per scenario.  A collective whose
    peer has died raises after two minutes instead of waiting for it."""
    import torch.distributed as dist
    job = torch.load(os.path.join(out_dir, "spec.pt"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    if job["device"] != "cpu":
        torch.cuda.set_device(0)
    for spec in job["specs"]:
        res = run_real_envs(spec, dist, rank) if spec["kind"] == "envs" else run_scenario(spec, job["device"], dist, rank)
        torch.save(res, os.path.join(out_dir, "%s_r%d.pt" % (spec["name"], rank)))
    dist.destroy_process_group()


_FAULTED = []


def launch(world, specs, out_dir, device):
    """Start ``world`` ranks as fresh child processes on ``specs`` and return {scenario name: [rank 0's result, rank 1's, ...]}.  Every
    child runs under its own limit and is killed at it; a child that ended on a signal or at its limit fails the caller and nothing is
    started after it, by this call or a later one."""
    if _FAULTED:
        raise RuntimeError("no ranks are started after %s" % _FAULTED[0])
    out_dir = str(out_dir)
    torch.save({"device": device, "specs": specs}, os.path.join(out_dir, "spec.pt"))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    flags = ["-s"] if sys.flags.no_user_site else []
    procs = [subprocess.Popen([sys.executable] + flags + ["-c", "import multi_rank_util as u; u.rank_main(%d, %d, %d, %r)"
                                                          % (rank, world, port, out_dir)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rank in range(world)]
    outs, late = [], False
    try:
        for p in procs:
            try:
                outs.append(p.communicate(timeout=CHILD_LIMIT)[0])
            except subprocess.TimeoutExpired:
                late = True
                for q in procs:                      # its peers wait for it in a collective: none of them goes on
                    if q.poll() is None:
                        q.kill()
                outs.append(p.communicate()[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    codes = [p.returncode for p in procs]
    tail = "\n".join("--- rank %d (exit %s)\n%s" % (r, c, o[-3000:]) for r, (c, o) in enumerate(zip(codes, outs)))
    if late or any(c < 0 for c in codes):
        _FAULTED.append("a %d-rank launch whose children ended %r%s" % (world, codes, " at the time limit" if late else ""))
        raise RuntimeError(_FAULTED[0] + "\n" + tail)
    assert all(c == 0 for c in codes), tail
    return {spec["name"]: [torch.load(os.path.join(out_dir, "%s_r%d.pt" % (spec["name"], r))) for r in range(world)] for spec in specs}


def run_single_then_ranks(specs_same, specs_own, world, out_dir, device):
    """the single process on every "same" scenario (in this process), then ONE launch of ``world`` ranks over the same rollouts and
    sample orders and over the "own" scenarios"""
    single = {}
    for spec in specs_same:
        single[spec["name"]] = res = run_scenario(spec, device)
        spec["rolls"], spec["orders"] = [x["roll"] for x in res["updates"]], [x["orders"] for x in res["updates"]]
    ranks = launch(world, specs_same + specs_own, out_dir, device)
    return {"single": single, "ranks": ranks, "specs": {s["name"]: s for s in specs_same + specs_own}}


# ---- "same": bit for bit ----
def assert_same_bits(a, b, what, count_factor=1):
    """Every parameter, both Adam moments, the step count, the rate sequence and what update() returned: the same bits in the results a
    and b.  The observation statistics: the same mean, variance and float form, b's count ``count_factor`` times a's."""
    assert len(a["updates"]) == len(b["updates"]) > 0 and a["fused"] == b["fused"]
    for k, (ua, ub) in enumerate(zip(a["updates"], b["updates"])):
        pa, pb = ua["post"], ub["post"]
        for key in ("params", "m", "v"):
            for name in PARAM_ORDER:
                assert torch.isfinite(pa[key][name]).all(), (what, k, key, name)
                assert torch.equal(pa[key][name], pb[key][name]), (what, k, key, name, (pa[key][name] - pb[key][name]).abs().max().item())
        assert pa["t"] == pb["t"] and pa["t"] > ua["pre"]["t"], (what, k, pa["t"], pb["t"])
        assert pa["lr"] == pb["lr"], (what, k, pa["lr"], pb["lr"])
        assert ua["lr_history"] == ub["lr_history"], (what, k, ua["lr_history"], ub["lr_history"])
        assert ua["stats"] == ub["stats"] and all(math.isfinite(x) for x in ua["stats"].values()), (what, k, ua["stats"], ub["stats"])
        for key in ("obs_norm", "cobs_norm"):
            assert (key in pa) == (key in pb), (what, key)
            if key in pa:
                sa, sb = pa[key]["state"], pb[key]["state"]
                assert torch.equal(sa[:-1], sb[:-1]) and torch.equal(pa[key]["norm"], pb[key]["norm"]), (what, k, key)
                assert sa[-1].item() > 0 and sb[-1].item() == count_factor * sa[-1].item(), (what, k, key, sa[-1].item(), sb[-1].item())


def decision(kl, d=SCHED["desired_kl"]):
    return "cut" if kl > 2.0 * d else ("rise" if 0.0 < kl < 0.5 * d else "keep")


def assert_rate_sequence_is_a_test_of_the_rule(single):
    """the one-process rate sequence holds a rise, a cut and a step that keeps the rate, and does not sit on a bound throughout"""
    hist = [h for u in single["updates"] for h in u["lr_history"]]
    lrs = [np.float32(LR)] + [np.float32(lr) for _, lr in hist]
    seen = set()
    for i, (kl, _) in enumerate(hist):
        moved = "rise" if lrs[i + 1] > lrs[i] else ("cut" if lrs[i + 1] < lrs[i] else "keep")
        if moved == decision(kl):                                   # (a rate held at a bound is no decision to keep it)
            seen.add(moved)
    assert seen == {"rise", "cut", "keep"}, (seen, hist)
    inside = [np.float32(SCHED["lr_min"]) < lr < np.float32(SCHED["lr_max"]) for lr in lrs[1:]]
    assert any(inside), hist
    return hist


# ---- "own": one float64 step of W ranks ----
def _flat(named):
    return np.concatenate([np.asarray(named[k].detach().double().numpy() if torch.is_tensor(named[k]) else named[k], np.float64).reshape(-1)
                           for k in PARAM_ORDER])


def _named(flat, like):
    out, o = {}, 0
    for k in PARAM_ORDER:
        n = like[k].numel()
        out[k] = flat[o:o + n].reshape(tuple(like[k].shape)); o += n
    return out


def reference_step(spec, pre, rolls, orders):
    """ONE optimiser step of W ranks in float64, from the state ``pre`` every rank held in front of it.  Per rank: the advantage
    normalised over the rank's own minibatch (adv_stats64), the gradient of the whole minibatch loss - its entropy term included -
    by float64 autograd (ppo_grad64), approx_kl and clip_frac (diag64).  Then the ranks' gradients summed and clip_adam64 with
    grad_scale = 1 / W, at the rate adapt_lr gives on the mean KL."""
    import ppo_diag_ref as dref
    from oracle.policy_ref import adv_stats64, clip_adam64, ppo_grad64
    from gym_roboy_amd.ppo import _flat_names
    da, dc, W = spec["da"], spec["dc"], len(rolls)
    pol = policy64(pre["params"], da, dc)
    net = Rows(pol, da, dc)
    gsum, pgs, vfs, diags = 0.0, [], [], []
    for roll, order in zip(rolls, orders):
        flat = {k: v.reshape(-1, *v.shape[2:]) for k, v in roll.items()}
        idx = order[:max(flat["obs"].shape[0] // spec["nminibatches"], 1)]
        rows = net_rows(flat["obs"][idx], pre.get("obs_norm"))
        if dc is not None:
            rows = torch.cat([rows, net_rows(flat["cobs"][idx], pre.get("cobs_norm"))], dim=1)
        mean, inv = adv_stats64(flat["adv"].numpy(), idx.numpy())
        adv = (flat["adv"][idx].double() - mean) * inv
        pg, vf = ppo_grad64(net, rows, flat["act"][idx].double(), adv, flat["logp"][idx].double(), flat["val"][idx].double(),
                            flat["ret"][idx].double(), CLIPRANGE, VF_COEF, ENT_COEF)
        gsum = gsum + _flat({k: p.grad for k, p in _flat_names(pol).items()})
        pgs.append(pg); vfs.append(vf)
        diags.append(dref.diag64(net, rows, flat["act"][idx], flat["logp"][idx], CLIPRANGE))
    kls = [d["approx_kl"] for d in diags]
    lr = np.float32(pre["lr"])
    if spec["lr_schedule"] is not None:
        lr = dref.adapt_lr(lr, sum(kls) / W, SCHED["desired_kl"], SCHED["lr_factor"], SCHED["lr_min"], SCHED["lr_max"])
    p0, m0, v0 = _flat(pre["params"]), _flat(pre["m"]), _flat(pre["v"])
    ls = sum(pre["params"][k].numel() for k in PARAM_ORDER[:-1])
    p1, m1, v1 = clip_adam64(p0, gsum, m0, v0, [(0, p0.shape[0])], float(lr), BETAS, ADAM_EPS, pre["t"] + 1, spec["max_grad_norm"], 1.0 / W,
                             0.0, (ls, ls + ACT))
    like = pre["params"]
    return {"params": _named(p1, like), "m": _named(m1, like), "v": _named(v1, like), "m0": _named(m0, like), "v0": _named(v0, like),
            "lr": lr, "pg": sum(pgs) / W, "vf": sum(vfs) / W, "kls": kls, "kl": sum(kls) / W, "diags": diags,
            "clip_frac": sum(d["clip_frac"] for d in diags) / W, "norm": float(np.sqrt(((gsum / W) ** 2).sum()))}


def reference_norm_of_first_step(spec, world):
    """the float64 norm of the first step's mean gradient, for a max_grad_norm on a chosen side of it"""
    from gym_roboy_amd.ppo import MlpPolicy, _flat_names
    p = MlpPolicy(spec["da"], ACT, critic_obs_dim=spec["dc"])
    p.load_state_dict(spec["policy_state"])
    params = {k: q.detach().clone() for k, q in _flat_names(p).items()}
    zeros = {k: torch.zeros_like(q) for k, q in params.items()}
    pre = {"params": params, "m": zeros, "v": zeros, "t": 0, "lr": LR}
    pol = policy64(params, spec["da"], spec["dc"])
    n = T * spec["n_envs"]
    rolls = [build_rollout(pol, spec["da"], spec["dc"], spec["n_envs"], 100000 * spec["seed"] + r, spec["kls"][0][r],
                           adv_shift=0.5 * r, adv_scale=1.0 + r) for r in range(world)]
    return reference_step(spec, pre, rolls, [torch.arange(n)] * world)["norm"]


def own_shard_scenarios(world, shapes, clip_sides=("never", "always")):
    """The "own" scenarios of a world size: per shape (name, da, dc, fused) one with max_grad_norm at four times the float64 norm of the
    first step's gradient - never clipped, the moments see the gradient's scale - and one at a quarter of it - always clipped, the
    coefficient is exercised."""
    specs = []
    for i, (name, da, dc, fused) in enumerate(shapes):
        for side in clip_sides:
            spec = scenario("own_w%d_%s_%s" % (world, name, side), "own", da, dc, n_envs=24, nminibatches=1, noptepochs=1, updates=3,
                            fused=fused, lr_schedule="adaptive", normalize_obs=True, kls=KLS[world], seed=10 * world + i)
            spec["clip_side"] = side
            spec["max_grad_norm"] = reference_norm_of_first_step(spec, world) * (4.0 if side == "never" else 0.25)
            specs.append(spec)
    return specs


def assert_union_moments(state, rows):
    """an ObsNorm state (float64: mean, var, count) against numpy's two-pass float64 moments of all the rows it merged, to the bound
    tests/test_obs_norm_gpu.py holds two runs of the statistics to"""
    x = np.concatenate([np.asarray(r, np.float64).reshape(-1, np.shape(r)[-1]) for r in rows])
    D = x.shape[1]
    state = np.asarray(state, np.float64)
    mean, var, count = state[:D], state[D:2 * D], state[-1]
    m, v = x.mean(0), x.var(0)
    assert count == x.shape[0], (count, x.shape[0])
    assert (np.abs(var - v) <= 1e-8 * v + 1e-12 * m ** 2).all(), (np.abs(var - v), v)
    assert (np.abs(mean - m) <= 1e-8 * np.sqrt(v) + 1e-12 * np.abs(m)).all(), (np.abs(mean - m), np.sqrt(v))


def assert_own_shards_match_float64(spec, results, say=print):
    """Every step of an "own" scenario against ``reference_step``, with the bounds of the module that tests each kernel alone
    (tests/test_policy_gpu.py: loss terms 1e-4, gradient 5e-4 of a parameter's largest entry; tests/test_policy_scale_gpu.py: M_TOL,
    V_TOL, parameters 2e-6 per step; tests/test_lr_schedule_gpu.py: approx_kl and clip_frac), and the statistics against the moments
    of every rank's rows.  Returns the worst errors seen {quantity: figure}."""
    from test_lr_schedule_gpu import _clip_frac_rounding
    from test_policy_scale_gpu import M_TOL, V_TOL
    W = len(results)
    B = T * spec["n_envs"] // spec["nminibatches"]
    worst = {"pg": 0.0, "vf": 0.0, "m": 0.0, "v": 0.0, "params": 0.0, "approx_kl": 0.0, "clip_frac": 0.0}
    d = SCHED["desired_kl"]
    clipped = set()
    for r in range(1, W):                                        # every rank came out of every step with the same bits
        assert_same_bits(results[0], results[r], (spec["name"], "rank 0 / rank %d" % r))
    for k in range(spec["updates"]):
        ups = [r["updates"][k] for r in results]
        pre, post, stats = ups[0]["pre"], ups[0]["post"], ups[0]["stats"]
        ref = reference_step(spec, pre, [u["roll"] for u in ups], [u["orders"][0] for u in ups])
        # the inputs: every KL, their mean and their sum clear of the rule's two thresholds; the decisions this update is there for
        for x in ref["kls"] + [ref["kl"], sum(ref["kls"])]:
            assert abs(x / (0.5 * d) - 1.0) > 0.01 and abs(x / (2.0 * d) - 1.0) > 0.01, (k, x)
        assert (decision(ref["kl"]), decision(ref["kls"][0]), decision(sum(ref["kls"]))) == DECISIONS[W][k], (k, ref["kls"])
        side = "never" if ref["norm"] < 0.5 * spec["max_grad_norm"] else ("always" if ref["norm"] > 2.0 * spec["max_grad_norm"] else "near")
        assert side == spec["clip_side"], (k, ref["norm"], spec["max_grad_norm"])
        clipped.update(("low",) if any(x["n_low"] for x in ref["diags"]) else ())
        clipped.update(("high",) if any(x["n_high"] for x in ref["diags"]) else ())
        assert sum(x["borderline"] for x in ref["diags"]) == 0
        # the rule: exactly the float32 statement on the float64 mean KL
        assert post["t"] == pre["t"] + 1
        assert np.float32(post["lr"]) == ref["lr"] and np.float32(stats["lr"]) == ref["lr"], (k, post["lr"], ref["lr"], ref["kls"])
        assert ups[0]["lr_history"][-1][1] == post["lr"]
        # loss terms and diagnostics: the means over the ranks
        err = {"pg": abs(stats["pg_loss"] - ref["pg"]) / max(1.0, abs(ref["pg"])), "vf": abs(stats["vf_loss"] - ref["vf"]) / max(1.0, abs(ref["vf"])),
               "approx_kl": abs(stats["approx_kl"] - ref["kl"]) / max(1.0, abs(ref["kl"])), "clip_frac": abs(stats["clip_frac"] - ref["clip_frac"])}
        tol_cf = sum(_clip_frac_rounding(B, x["clip_frac"], 256) for x in ref["diags"]) / W + 2.0 ** -24 * (W + 1) * ref["clip_frac"]
        # (the entropy is the log-std's alone, the same on every rank: the torch path reports it in front of the step, the fused one behind it)
        log_std = (post if results[0]["fused"] else pre)["params"]["log_std"].double()
        entropy = float((0.5 + 0.5 * math.log(2 * math.pi) + log_std).sum())
        assert abs(stats["entropy"] - entropy) < 1e-5 * max(1.0, abs(entropy)), (k, stats["entropy"], entropy)
        # the moments' increments and the parameters
        for name in PARAM_ORDER:
            for key, m0 in (("m", "m0"), ("v", "v0")):
                want = ref[key][name] - ref[m0][name]
                got = post[key][name].double().numpy() - ref[m0][name]
                err[key] = max(err.get(key, 0.0), np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))
            err["params"] = max(err.get("params", 0.0), np.abs(post["params"][name].double().numpy() - ref["params"][name]).max())
        say("%s update %d: norm %.4g against max_grad_norm %.4g, KLs %s -> lr %.6g; errors pg %.3g vf %.3g approx_kl %.3g clip_frac %.3g "
            "(allowed %.3g) m %.3g v %.3g params %.3g" % (spec["name"], k, ref["norm"], spec["max_grad_norm"],
                                                        ["%.4g" % x for x in ref["kls"]], ref["lr"], err["pg"], err["vf"], err["approx_kl"],
                                                        err["clip_frac"], tol_cf, err["m"], err["v"], err["params"]))
        for key in worst:
            worst[key] = max(worst[key], float(err[key]))
        assert err["pg"] < 1e-4 and err["vf"] < 1e-4, (k, err)
        assert err["approx_kl"] <= 1e-4 and err["clip_frac"] <= tol_cf, (k, err, tol_cf)
        assert err["m"] <= 5e-4 + M_TOL, (k, err)
        assert err["v"] <= 2 * 5e-4 + V_TOL, (k, err)
        assert err["params"] <= 2e-6, (k, err)
    assert clipped == {"low", "high"}                            # ratios left the clip range on both sides somewhere
    # the statistics: the moments of every rank's rows of every update
    last = results[0]["updates"][-1]["post"]
    for key, rows in (("obs_norm", "obs"), ("cobs_norm", "cobs")):
        if key in last:
            assert_union_moments(last[key]["state"].numpy(), [u["roll"][rows].numpy() for r in results for u in r["updates"]])
    assert ("cobs_norm" in last) == (spec["dc"] is not None) and "obs_norm" in last
    return worst
