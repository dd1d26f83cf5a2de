"""ms per learner.train call (one optimisation step: denominators, unroll of both nets, loss, backward, clip + Adam) of Cleanup-5 at
B = 16 episodes of 101 time slots, with and without consider_others_inc, eager and with the train step captured as hipGraphs, and
whether the step took the fused loss kernel.

    python tools/learner_option_iters.py [--iters 30] [--warmup 5] [--root TREE]

--root: import the package from another checkout (e.g. the parent commit's, to measure "before" with the same script).  The batch is
the synthetic one of tests/test_hip_learner_path.py (rewards, cleaning, incentives of all kinds, early termination).
"""
import argparse
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from types import SimpleNamespace
    import torch as th
    from homophily_marl_amd.controllers import REGISTRY as mac_REGISTRY
    from homophily_marl_amd.learners import REGISTRY as le_REGISTRY
    from tests.test_hip_learner_path import _random_learner_batch
    batch, base, _ = _random_learner_batch(16, 100, 5, "cleanup", seed=3)
    for graph in (False, True):
        for others in (False, True):
            args = SimpleNamespace(**vars(base.args))
            args.train_graph, args.consider_others_inc = graph, others
            mac = mac_REGISTRY[args.mac](batch.scheme, {"agents": 5}, args).cuda()
            mac.agent.load_state_dict(base.mac.agent.state_dict())
            learner = le_REGISTRY[args.learner](mac, batch.scheme, SimpleNamespace(log_stat=lambda *x, **k: None, console_logger=None), args)
            learner.cuda()
            learner.target_mac.load_state(base.target_mac)
            learner.log_stats_t = float("inf")          # no log interval inside the timed calls
            for _ in range(a.warmup):
                learner.train(batch, 0, 0)
            th.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                learner.train(batch, 0, 0)
            th.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / a.iters
            print("consider_others_inc %-5s  %-6s  fused %-5s  captured %-5s  %8.3f ms / train call  (%d calls, B 16, 101 slots, Cleanup-5)"
                  % (others, "graph" if graph else "eager", learner._fused(batch), learner._graph is not None, ms, a.iters), flush=True)
            del learner, mac
            th.cuda.empty_cache()


if __name__ == "__main__":
    main()
