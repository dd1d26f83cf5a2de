"""CPU suite: ops.capture keeps Python's cyclic collector out of a graph capture -- dead cycles are finalised before the capture
begins, none while it runs, and the collector's state is put back however the capture ends."""
import gc

import pytest
import torch as th

from homophily_marl_amd import ops


class _Owner:
    """one half of a dead reference cycle whose finaliser records when it ran"""

    def __init__(self, log):
        self.log, self.me = log, self

    def __del__(self):
        self.log.append("finalised")


class _FakeCapture:
    def __init__(self, log, fail=False):
        self.log, self.fail = log, fail

    def __enter__(self):
        self.log.append("begin")
        if self.fail:
            raise RuntimeError("capture_begin failed")

    def __exit__(self, *exc):
        self.log.append("end")
        return False


@pytest.mark.parametrize("gc_on", [True, False])
def test_cycles_are_collected_before_the_capture_and_none_inside(monkeypatch, gc_on):
    log = []
    monkeypatch.setattr(th.cuda, "graph", lambda g, **kw: _FakeCapture(log))
    was = gc.isenabled()
    try:
        gc.enable() if gc_on else gc.disable()
        _Owner(log)                                             # dead at once, but only the cyclic collector can free it
        with ops.capture(object(), capture_error_mode="thread_local"):
            assert not gc.isenabled()
            _Owner(log)
            for _ in range(3):                                  # enough allocations for several young-generation thresholds
                junk = [[i] for i in range(5000)]
            del junk
            log.append("captured")
        assert gc.isenabled() == gc_on
        gc.collect()
        assert log == ["finalised", "begin", "captured", "end", "finalised"]
    finally:
        gc.enable() if was else gc.disable()


def test_the_collector_comes_back_when_the_capture_fails(monkeypatch):
    log = []
    was = gc.isenabled()
    gc.enable()
    try:
        monkeypatch.setattr(th.cuda, "graph", lambda g, **kw: _FakeCapture(log, fail=True))
        with pytest.raises(RuntimeError, match="capture_begin"):
            with ops.capture(object()):
                pass
        assert gc.isenabled()
        monkeypatch.setattr(th.cuda, "graph", lambda g, **kw: _FakeCapture(log))
        with pytest.raises(ValueError):
            with ops.capture(object()):
                raise ValueError("a launch failed")
        assert gc.isenabled() and log == ["begin", "begin", "end"]
    finally:
        gc.enable() if was else gc.disable()
