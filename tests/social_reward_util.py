"""The independent statement of the two reward models (include/ssd_hip_reward.h: ssd_social_reward) in numpy loops, written from the
formulas and not by calling ops -- a helper, no test in it.  Every operation is one np.float32 operation (one rounding); the sums over
the partners run in ascending j from 0 and skip the agent itself (`descending`: the same sums in descending j, to show that the test
inputs can tell the two orders apart)."""
import copy

import numpy as np

f32 = np.float32
DRAWS = np.array([0, 0, 0, 1, 1, -1, -50], dtype=np.float32)         # the env's rewards: apple +1, hit by a beam -50, firing -1


def scalars(model, n, alpha=5.0, beta=0.05, decay=0.96525, rho=0.5):
    """(p0, p1, p2): the keys rounded to f32, then ONE f32 operation each"""
    if model == "inequity_aversion":
        return f32(alpha) / f32(n - 1), f32(beta) / f32(n - 1), f32(decay)
    return f32(1) - f32(rho), f32(rho) / f32(n - 1), f32(0)


def shaped(model, reward, p, acc=None, descending=False):
    """reward f32 [N, t_slots, n] -> shaped f32 [N, t_slots, n] (slot t_slots - 1 is 0); acc f64 [N, n, 3] += the three columns, one
    term per slot in ascending t."""
    reward = np.asarray(reward, dtype=np.float32)
    N, T1, n = reward.shape
    p0, p1, p2 = (f32(x) for x in p)
    out = np.zeros((N, T1, n), dtype=np.float32)
    order = range(n - 1, -1, -1) if descending else range(n)
    for b in range(N):
        e = np.zeros(n, dtype=np.float32)
        for t in range(T1 - 1):
            r = reward[b, t]
            if model == "inequity_aversion":
                for j in range(n):
                    e[j] = f32(f32(p2 * e[j]) + r[j])
            for i in range(n):
                if model == "inequity_aversion":
                    envy, guilt = f32(0), f32(0)
                    for j in order:
                        if j != i:
                            envy = f32(envy + max(f32(e[j] - e[i]), f32(0)))
                            guilt = f32(guilt + max(f32(e[i] - e[j]), f32(0)))
                    second, third = f32(p0 * envy), f32(p1 * guilt)
                    u = f32(f32(r[i] - second) - third)
                else:
                    s = f32(0)
                    for j in order:
                        if j != i:
                            s = f32(s + r[j])
                    second, third = f32(p1 * s), f32(0)
                    u = f32(f32(p0 * r[i]) + second)
                out[b, t, i] = u
                if acc is not None:
                    acc[b, i, 0] += np.float64(u)
                    acc[b, i, 1] += np.float64(second)
                    acc[b, i, 2] += np.float64(third)
    return out


def logged_mean(acc, column, count):
    """the runner's logged mean of one accumulator column: the cells added in ascending (env, agent), left to right from 0, in f64,
    then ONE division by the count of (rollout, env, slot < T, agent)"""
    total = np.float64(0)
    for b in range(acc.shape[0]):
        for i in range(acc.shape[1]):
            total = total + np.float64(acc[b, i, column])
    return float(total / np.float64(count))


def draw(N, t_slots, n, seed):
    """rewards of the draw family {0, 0, 0, 1, 1, -1, -50}; the bootstrap slot carries a value no result may depend on"""
    rng = np.random.default_rng(seed)
    r = DRAWS[rng.integers(0, len(DRAWS), size=(N, t_slots, n))]
    r[:, -1] = 7.0
    return r


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


# ---- the learner comparison: key on against the key-off learner fed the shaped field ------------------------------------------------------
RAW = "reward_env_paid"


def add_field(batch, model="inequity_aversion", **keys):
    """give the batch the storage field "reward_model": the util's shaping of its own rewards (the batch is one rollout of B envs)"""
    import torch as th
    r = batch["reward"].cpu().numpy()
    if not r[:, :-1].any():      # the recorded episodes of the learner fixtures are short random play that earned nothing: a model has
        r = draw(*r.shape, seed=5)                                    # nothing to shape there, so the batch is paid from the draw family
        batch.data.transition_data["reward"].copy_(th.as_tensor(r))
    s = shaped(model, r, scalars(model, r.shape[-1], **keys))
    batch.scheme["reward_model"] = dict(batch.scheme["reward"])
    batch.data.transition_data["reward_model"] = th.as_tensor(s).to(batch.device)
    assert not np.array_equal(s[:, :-1], r[:, :-1])
    return batch


class _EnvPaid:
    """a batch as the controller reads it, whose "reward" is what the env paid"""

    def __init__(self, batch):
        self._batch = batch

    def __getitem__(self, key):
        return self._batch[RAW if key == "reward" else key]

    def __getattr__(self, name):
        return getattr(self._batch, name)


def key_off_twin(batch_on, learner_off):
    """The comparison of the issue, with its inputs mended: the key-off learner is fed a batch whose `reward` IS the shaped field.  The
    incentive head's per-receiver features carry r_j with every input set (homophily_agent.py: unroll_other), so under obs_reward: False
    the two runs' network inputs still differ unless the key-off run's CONTROLLERS are shown what the env paid; the raw rewards ride
    along under another name and the two controllers of the key-off learner (and only they: its loss reads `reward`, the shaped
    values) read them.  Nothing of the key-on run is touched."""
    ref = copy.deepcopy(batch_on)
    td = ref.data.transition_data
    td[RAW] = td["reward"]
    td["reward"] = td.pop("reward_model")
    ref.scheme.pop("reward_model", None)
    for mac in (learner_off.mac, learner_off.target_mac):
        inner = mac.unroll_shared
        mac.unroll_shared = lambda b, inner=inner: inner(_EnvPaid(b))
    return ref


class NoWeights:
    """a learner fixture without its recorded weights (they are shaped for the shipped input set): tests.learner_util.build then keeps
    the random initialisation, which the caller seeds"""

    def __init__(self, z):
        self._z, self.files = z, [k for k in z.files if not k.startswith("w_")]

    def __getitem__(self, key):
        return self._z[key]


def build_seeded(z, meta, device="cpu", seed=0, code_obs=False, **overrides):
    import torch as th
    from tests.learner_util import build
    th.manual_seed(seed)
    return build(NoWeights(z), meta, device=device, overrides=overrides, code_obs=code_obs)
