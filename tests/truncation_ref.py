"""TEST HELPER: episode-end codes and value bootstrapping of truncated episodes restated from the definition alone.

Codes: 0 not done, 1 terminated (the goal was reached - it wins where the time limit falls on the same step), 2 truncated (the time
limit alone ended the episode).  The coded recurrence in float64, the code patterns of the kernel tests, and the scenario that puts every
code - and the coincidence of goal and time limit - into a short run of the fused env step."""
import numpy as np

NONE, TERMINATED, TRUNCATED = 0, 1, 2


def gae_boot64(rew, val, code, last_val, gamma, lam):
    """adv, ret [T, N] in float64: oracle/policy_ref.py's gae64 with done_t = (code_t != 0) and, where code_t == 2, the reward
    rew_t + gamma val_t - the value of the state the episode was cut at stands in for the return that the time limit cut off."""
    rew, val = np.asarray(rew, np.float64), np.asarray(val, np.float64)
    code = np.asarray(code)
    next_value = np.asarray(last_val, np.float64)
    T = rew.shape[0]
    adv = np.zeros_like(rew)
    last = np.zeros_like(next_value)
    for t in range(T - 1, -1, -1):
        nonterminal = np.where(code[t] != 0, 0.0, 1.0)
        r = np.where(code[t] == TRUNCATED, rew[t] + gamma * val[t], rew[t])
        delta = r + gamma * next_value * nonterminal - val[t]
        last = delta + gamma * lam * nonterminal * last
        adv[t] = last
        next_value = val[t]
    return adv, adv + val


def boot_extra_bound(r_tilde, val, code, gamma):
    """What the two extra roundings of a truncated step - fl32(gamma32 val) and fl32(r~ + that) - may add to adv / ret beyond the
    parent recurrence's own error: each is within 2^-24 of its result's magnitude, they enter delta_t of a step with nonterminal = 0
    (nothing behind it feeds that step), and delta_t reaches the advantages before it with the weights (gamma lam)^k <= 1 until the
    previous episode end - one source per episode, never summed.  So: 2^-24 max over the truncated steps of |gamma v| + |r~ + gamma v|."""
    m = np.asarray(code) == TRUNCATED
    if not m.any():
        return 0.0
    gv = gamma * np.asarray(val, np.float64)[m]
    return 2.0 ** -24 * float((np.abs(gv) + np.abs(np.asarray(r_tilde, np.float64)[m] + gv)).max())


def gae_boot_magnitude(rew, val, code, last_val, gamma, lam):
    """A [T, N]: the coded recurrence on absolute values - |r| (+ gamma |v| where truncated) + gamma |V_next| nt + |v| + gamma lam nt
    A_next - the magnitude every rounding of a float32 evaluation of adv_t is relative to."""
    rew, val = np.abs(np.asarray(rew, np.float64)), np.abs(np.asarray(val, np.float64))
    code = np.asarray(code)
    nxt = np.abs(np.asarray(last_val, np.float64))
    A = np.zeros_like(rew)
    a = np.zeros_like(nxt)
    for t in range(rew.shape[0] - 1, -1, -1):
        nt = np.where(code[t] != 0, 0.0, 1.0)
        a = rew[t] + np.where(code[t] == TRUNCATED, gamma * val[t], 0.0) + gamma * nxt * nt + val[t] + gamma * lam * nt * a
        A[t] = a
        nxt = val[t]
    return A


def gae_boot32_bound(T, A):
    """20 T 2^-24 A: a float32 evaluation rounds at most ten times per step (gamma and gamma lam to float32, gamma v, the bootstrap's
    sum, gamma V_next, delta's sum and difference, gamma lam adv, its sum, adv + v), each within 2^-24 of a quantity A bounds, and a
    step's error reaches the steps before it with weights <= 1: 10 T 2^-24 A to first order, doubled for the higher orders - the way
    tests/reward_norm_ref.py's carry_bound counts the scan's two roundings per step as 4 T 2^-53 A."""
    return 20.0 * T * 2.0 ** -24 * A


CODE_PATTERNS = ("half", "every_done_truncated", "truncated_last_step", "truncated_first_step")


def codes_of(done, kind, rng):
    """int32 codes from 0 / 1 done flags [T, N].  half: every done becomes a 2 with probability 1/2; every_done_truncated; a row of 2s
    at t = T - 1 / at t = 0 on top of `half`."""
    done = np.asarray(done, np.int32)
    code = np.where((done != 0) & (rng.random(done.shape) < 0.5), TRUNCATED, done).astype(np.int32)
    if kind == "every_done_truncated":
        code = np.where(done != 0, TRUNCATED, 0).astype(np.int32)
    elif kind == "truncated_last_step":
        code[-1] = TRUNCATED
    elif kind == "truncated_first_step":
        code[0] = TRUNCATED
    else:
        assert kind == "half"
    return code


# ---- the env scenario: every code within 12 steps of a 5-step time limit ----
MAX_LEN, STEPS = 5, 12


def scenario(n, n_q, n_t, goal0, seed=11):
    """-> (goal [n, n_q], step_num [n] uint32, actions [STEPS, n, n_t], groups [n]) for envs that were just reset to the zero pose with
    the goals goal0.  Env i of group i % 3:
      0  'goal':     its goal is the zero pose it rests at and its first action is the rest command - it reaches the goal at step 0;
      1  'coincide': the same, with the step counter at the limit - goal and time limit fall on step 0 (terminated wins);
      2  'free':     the drawn goal, random actions - the time limit ends its episodes at steps 4 and 9.
    Behind an episode end every env runs on with random actions towards a redrawn goal: the time limit ends that episode five steps on."""
    rng = np.random.default_rng(seed)
    groups = np.arange(n) % 3
    goal = np.array(goal0, np.float32)
    goal[groups != 2] = 0.0
    step_num = np.where(groups == 1, MAX_LEN, 1).astype(np.uint32)
    actions = rng.uniform(-1.0, 1.0, (STEPS, n, n_t)).astype(np.float32)
    actions[0, groups != 2] = 0.0
    return goal, step_num, actions, groups


def expected_codes(done, rew):
    """The codes as the twin (an env without the option, goal bonus on) shows them: every reward term but the bonus is <= -1, so the
    reward is positive exactly when the goal was reached."""
    done, rew = np.asarray(done, bool), np.asarray(rew)
    return np.where(done & (rew > 0), TERMINATED, np.where(done, TRUNCATED, NONE)).astype(np.uint32)


def assert_every_code_occurs(codes, groups, at_least=8):
    """codes [STEPS, n]: each of 0, 1, 2 in at least `at_least` envs, the coincidence envs terminated at step 0 - and truncated later"""
    codes = np.asarray(codes)
    for c in (NONE, TERMINATED, TRUNCATED):
        assert (codes == c).any(axis=0).sum() >= at_least, (c, (codes == c).any(axis=0).sum())
    co = groups == 1
    assert co.sum() >= at_least and (codes[0, co] == TERMINATED).all()
    assert (codes[0, groups == 0] == TERMINATED).all() and (codes[0, groups == 2] == NONE).all()
    # their second episode, five steps old (all but the odd env that reaches its redrawn goal on the way)
    assert (codes[MAX_LEN, groups != 2] == TRUNCATED).sum() >= max(at_least, (groups != 2).sum() - 2)
    assert (codes[MAX_LEN - 1, groups == 2] != NONE).sum() >= at_least
