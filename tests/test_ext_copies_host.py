"""The wrapper-side count of recorded external copies (safe_gossip_amd
ExtCopies), which sliced and sharded networks check a whole batch against
before any engine applies a part of it: the engine's rule (gs_engine.cpp
ext_copies, gs_common.h kExtCopiesMax) restated on the host.  No GPU."""
import pytest


def test_ext_copies_bound(engine):
    ec = engine.ExtCopies()
    top = engine.EXT_COPIES_MAX
    assert top == 96
    full = [(7, 3, 1000 + i) for i in range(top)]
    ec.commit(ec.check(full))
    # a peer that has a copy may replace it; other nodes and rumors count apart
    ec.commit(ec.check([(7, 3, 1000), (7, 4, 2000), (8, 3, 2000)]))
    with pytest.raises(engine.DeviceError, match="status -5"):
        ec.check([(9, 9, 1), (7, 3, 2000)])
    # the refused batch left nothing behind: (9, 9) still takes its 96
    ec.commit(ec.check([(9, 9, 10 + i) for i in range(top)]))
    # within one batch: the same peer twice is one copy, the 97th peer is refused
    with pytest.raises(engine.DeviceError, match="status -5"):
        ec.check([(1, 0, i) for i in range(top + 1)])
    ec.commit(ec.check([(1, 0, i % top) for i in range(3 * top)]))
    ec.reset()  # a new round
    ec.commit(ec.check([(7, 3, 2000)]))
