"""_native.gc_paused(): the block every stream capture of the package runs in.  No cyclic collection may start between the launches
of a capture (the destructors of earlier work's dead cycles make runtime calls a capture does not allow), and the collector's
state is the caller's again afterwards - also when the block raises, and when the collector was off to begin with.  No GPU."""
import gc
import os
import re

import pytest

import mdr_amd._native as nat

PACKAGE = os.path.dirname(os.path.abspath(nat.__file__))


class _Cycle:
    freed = 0

    def __init__(self):
        self.me = self

    def __del__(self):
        _Cycle.freed += 1


def test_no_cycle_is_collected_inside_the_block_and_all_of_them_after_it():
    gc.collect()
    _Cycle.freed = 0
    assert gc.isenabled()
    with nat.gc_paused():
        assert not gc.isenabled()
        for _ in range(5000):      # far past the allocation count at which the collector would start
            _Cycle()
        assert _Cycle.freed == 0
    assert gc.isenabled()
    gc.collect()
    assert _Cycle.freed == 5000


def test_the_collector_comes_back_when_the_block_raises():
    with pytest.raises(RuntimeError):
        with nat.gc_paused():
            raise RuntimeError("capture failed")
    assert gc.isenabled()


def test_a_collector_that_was_off_stays_off():
    gc.disable()
    try:
        with nat.gc_paused():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()


def test_every_capture_of_the_package_runs_in_the_block():
    sites = []
    for name in sorted(os.listdir(PACKAGE)):
        if name.endswith(".py"):
            for line in open(os.path.join(PACKAGE, name)):
                if re.search(r"with .*torch\.cuda\.graph\(", line):
                    sites.append((name, line.strip()))
    assert len(sites) >= 3, sites
    assert all("nat.gc_paused()" in line for _, line in sites), sites
