"""Epsilon schedule (reference: src/components/epsilon_schedules.py:4-25)."""
import math


class DecayThenFlatSchedule:
    def __init__(self, start, finish, time_length, decay="exp"):
        self.start, self.finish, self.time_length, self.decay = start, finish, time_length, decay
        self.delta = (start - finish) / time_length
        if decay == "exp":
            self.exp_scaling = -time_length / math.log(finish) if finish > 0 else 1

    def eval(self, T):
        if self.decay == "linear":
            return max(self.finish, self.start - self.delta * T)
        if self.decay == "exp":
            return min(self.start, max(self.finish, math.exp(-T / self.exp_scaling)))
        raise ValueError(self.decay)


def ladder_exponents(alpha, env_id_base, n_env, total):
    """The exponents of the per-env epsilon ladder (Ape-X / R2D2; config key epsilon_ladder_alpha) for the envs env_id_base ..
    env_id_base + n_env - 1 of a job of `total` envs: env g explores at eps ** (1 + alpha * g / (total - 1)) -- env 0 at the scheduled
    rate, env total - 1 at eps ** (1 + alpha); a job of one env has the exponent 1.  Formed in float64 from the GLOBAL env id and rounded
    to float32 (numpy array [n_env]), so that the shards of a job hold the slices of the unsharded vector.  No device is involved."""
    import numpy as np
    alpha, base, n_env, total = float(alpha), int(env_id_base), int(n_env), int(total)
    if n_env < 1 or base < 0 or base + n_env > total:
        raise ValueError("ladder_exponents: envs %d .. %d outside a job of %d envs" % (base, base + n_env - 1, total))
    g = np.arange(base, base + n_env, dtype=np.float64)
    if total == 1:
        return np.ones(1, dtype=np.float32)
    return (1.0 + alpha * g / float(total - 1)).astype(np.float32)
