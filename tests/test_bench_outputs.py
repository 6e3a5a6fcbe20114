"""bench.py's plain run, --full and --dump-outputs.

A plain run keeps only the legs the headline needs (no CPU legs, no spread
run, no live PMC children); --full switches them back on.  --dump-outputs
writes the observers of the network as the last timed round left it: checked
here on a fake network (sampling, number formats, size) and on the GPU against
a second network driven through the same rounds.
"""
import os

import numpy as np
import pytest

import bench


def test_plain_run_is_lean():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu_baseline and a.no_spread and a.pmc == "off"
    f = bench.parse(["--gpus", "1", "--full"])
    assert not f.no_cpu_baseline and not f.no_spread and f.pmc == "auto"
    g = bench.parse(["--full", "--no-spread", "--pmc", "off"])
    assert not g.no_cpu_baseline and g.no_spread and g.pmc == "off"
    # the live PMC children of a --full run are plain runs
    assert bench.parse(["--no-cpu-baseline", "--no-spread", "--pmc", "off"]).full is False


def u64_of(limbs):
    """(S, 4w) f32 16-bit limbs, low first -> (S, w) u64."""
    return np.ascontiguousarray(limbs.astype(np.uint16)).view(np.uint64)


class FakeNet:
    def __init__(self, n, R):
        self.n, self.R, self.kw = n, R, (R + 63) // 64
        rng = np.random.default_rng(7)
        self.st = rng.integers(0, 1 << 40, size=(n, 5), dtype=np.uint64)
        self.kn = rng.integers(0, 1 << 64, size=(n, self.kw), dtype=np.uint64)
        self.dg = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)

    def known_counts(self):
        return 123456789012, 42

    def statistics_all(self):
        return self.st

    def known_all(self):
        return self.kn

    def known_popcounts(self):
        return np.arange(self.n, dtype=np.uint32) % (self.R + 1)

    def state_digest(self):
        return self.dg


@pytest.mark.parametrize("n,R", [(1000, 256), (bench.DUMP_SAMPLE + 12345, 256), (70000, 4096)])
def test_dump_outputs_files(tmp_path, n, R):
    net = FakeNet(n, R)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(net, "single", d1, 0x5AFE6055)
    bench.dump_outputs(net, "single", d2, 0x5AFE6055)
    names = sorted(os.listdir(d1))
    assert names == sorted(x + ".npy" for x in ("known_counts", "sample_nodes", "statistics", "known_popcounts",
                                                "known_words", "state_digest"))
    assert sum(os.path.getsize(os.path.join(d1, f)) for f in names) <= 64 << 20
    out = {f[:-4]: np.load(os.path.join(d1, f)) for f in names}
    for f in names:  # same arguments, same files
        np.testing.assert_array_equal(out[f[:-4]], np.load(os.path.join(d2, f)))
        assert out[f[:-4]].dtype in (np.float32, np.float64)
    idx = out["sample_nodes"].astype(np.int64)
    assert len(idx) == bench.dump_sample_size(n, R) and len(np.unique(idx)) == len(idx)
    assert len(idx) == (n if n == 1000 else bench.DUMP_SAMPLE if R == 256 else 57614)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    np.testing.assert_array_equal(out["known_counts"], [123456789012, 42])
    np.testing.assert_array_equal(out["statistics"].astype(np.uint64), net.st[idx])
    np.testing.assert_array_equal(out["known_popcounts"].astype(np.uint32), net.known_popcounts()[idx])
    np.testing.assert_array_equal(u64_of(out["known_words"]), net.kn[idx])
    np.testing.assert_array_equal(u64_of(out["state_digest"])[:, 0], net.dg[idx])


@pytest.mark.gpu
def test_dump_outputs_match_network(engine, tmp_path):
    """The dumped arrays are the observers of a network after exactly
    --warmup rounds of epoch 0, a clear, and --steps rounds of epoch 1."""
    import torch
    n, R, K, W = 3001, 70, 6, 2  # two known-words per node, neither n nor R a multiple of 64
    args = bench.parse(["--gpus", "1", "--nodes", str(n), "--rumors", str(R), "--steps", str(K), "--warmup", str(W),
                        "--dump-outputs", str(tmp_path)])
    torch.cuda.set_device(0)
    run = bench.run_mode(args, "single", 1, 0, 0, None, engine, np, torch, with_spread=False)
    assert run["spread"] is None and len(run["kt"]) == K - 1
    out = {f[:-4]: np.load(str(tmp_path / f)) for f in os.listdir(str(tmp_path))}

    net = engine.Network(n, R, seed=args.seed, epoch=0, device=0)
    try:
        bench.inject_all(net, 0)
        for _ in range(W):
            net.next_round(report=False)
        net.clear(1)
        bench.inject_all(net, 1)
        for _ in range(K):
            net.next_round(report=False)
        assert net.round == K
        np.testing.assert_array_equal(out["sample_nodes"], np.arange(n))
        np.testing.assert_array_equal(out["known_counts"], net.known_counts())
        st = net.statistics_all()
        assert st[:, 0].max() == K  # Statistics.rounds: the timed rounds, no more
        np.testing.assert_array_equal(out["statistics"].astype(np.uint64), st)
        np.testing.assert_array_equal(out["known_popcounts"].astype(np.uint32), net.known_popcounts())
        np.testing.assert_array_equal(u64_of(out["known_words"]), net.known_all())
        np.testing.assert_array_equal(u64_of(out["state_digest"])[:, 0], net.state_digest())
        assert 0 < out["known_counts"][0] < n * R  # mid-dissemination: the arrays are not trivial
    finally:
        net.close()
