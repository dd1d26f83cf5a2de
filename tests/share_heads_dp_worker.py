"""One rank of the data-parallel share_heads test (tests/test_share_heads_host.py; started by tests/share_heads_util.run_ranks):
    python -m tests.share_heads_dp_worker RANK WORLD PORT SHARE OUTDIR
Two optimisation steps of the tensor-op learner on this rank's shard of learner_cleanup5.npz over gloo, CPU tensors.  The tie comes
after the gradient all-reduce (clip_and_step), so every rank holds the same tied gradient.  Writes OUTDIR/rank<R>.npz."""
import os
import sys
from datetime import timedelta

import numpy as np
import torch as th
import torch.distributed as dist


def main():
    rank, world, port, share, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    th.set_num_threads(1)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
    from tests import share_heads_util as U
    from tests.learner_util import param_checksums
    per = 4 // world
    batch, mac, learner, seen = U.fixture_learner(share, sl=slice(rank * per, (rank + 1) * per))
    assert learner.distributed and not learner._fused(batch)
    grads, inner = [], learner.clip_and_step

    def clip_and_step():
        inner()
        grads.append(learner._flat_grad.detach().clone())            # after the step: the tied gradient the optimisers saw
    learner.clip_and_step = clip_and_step
    rec = dict(sums=[], sqs=[], heads=[])
    for step in range(2):
        learner.cal_loss_and_step(batch)
        U.assert_invariant(mac, learner, U.TAGS[share], "rank %d step %d" % (rank, step))
        for key, v in zip(("sums", "sqs", "heads"), param_checksums(mac)):
            rec[key].append(v)
    state = [th.cat([p.detach().reshape(-1) for p in mac.parameters()])]
    for opt in (learner.optimiser_env, learner.optimiser_inc):
        for key in ("exp_avg", "exp_avg_sq"):
            state.append(th.cat([opt.state[p][key].reshape(-1) for p in opt.param_groups[0]["params"]]))
    np.savez(os.path.join(out, "rank%d.npz" % rank), flat=th.cat(state).numpy(), grads=th.stack(grads).numpy(),
             **{k: np.stack(v) for k, v in rec.items()})
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
