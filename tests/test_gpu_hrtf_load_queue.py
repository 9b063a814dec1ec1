"""k_hrtf_multi issues the same vector-memory operations on every path through a source trip: the request for the next
source's rows is unconditional (on a wave's very last trip it asks again for the wave's first row and throws it away),
and with history in LDS a wave stages its history rows in the prologue and writes them back in the last block.  None
of that may change a bit: a batched run against the ordered mode, mixes and peaks of every callback (a later callback
reads the history an earlier launch wrote back, so the write-back is compared too), at the shapes where the changed
code takes another path:
  * sources per wave (2048 waves from n = 2048 on): exactly 1, a mix of 1 and 2, exactly HIST_ROWS (history in LDS),
    HIST_ROWS + 1 (history through memory) -- HIST_ROWS is 6, 5, 4, 3 at F = 512, 384, 256, 128;
  * F = 128 at n = 128: the smallest list that batches at all (sixteen workgroups, one source per wave);
  * depth 2 (the shortest launch the context issues: its first block stages the history, its second writes it back)
    and depth 16, over T = 17 callbacks: eight launches of two plus one left over at depth 2, one launch of full depth
    plus one left over at depth 16 (a single callback left over runs k_hrtf_uni on the history the launch wrote back);
  * draining playbacks (exact peaks: the flagged path) on the first source of some waves and the last source of
    others, so that path meets the staged history and the thrown-away request; one run with every source flagged;
  * a device publish inside a batch, and none at all.
One case per F is compared with the oracle as well, at the suite's tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_ALL = 17
DIRS = 48
# (F, n): see above
SHAPES = [
    (512, 2048), (512, 2051), (512, 12288), (512, 14336),
    (384, 10240), (384, 12288),
    (256, 8192), (256, 10240),
    (128, 128), (128, 6144), (128, 6147), (128, 8192),
]
PUBLISH = {"no_publish": (), "publish_inside_a_batch": (1, 6, 11)}


def _wave_ends(n):
    """First and last list entry of every wave (gas_hrtf_wave.h wave_range over the launch's waves)."""
    wgs = max(min((n + 7) // 8, 256), (n + 511) // 512)
    waves = wgs * 8
    base, rem = divmod(n, waves)
    gw = np.arange(waves)
    first = gw * base + np.minimum(gw, rem)
    last = first + base + (gw < rem) - 1
    return first, last


def _draining(n):
    first, last = _wave_ends(n)
    return np.unique(np.concatenate([first[0::3], last[1::3]]))


_POOL = {}


def _inputs(n, F):
    """Three source buffers (used in turn) and four parameter sets per shape, drawn once."""
    from godot_audio_spatializer_amd import synth

    if (n, F) not in _POOL:
        rng = np.random.default_rng(1000 + n + F)
        srcs = [synth.draw_sources(rng, n, F) for _ in range(3)]
        psets = [synth.draw_params(rng, n, dirs=DIRS, frames=F) for _ in range(4)]
        _POOL.clear()  # one shape's inputs at a time (the cases of a shape run together)
        _POOL[(n, F)] = (srcs, psets)
    return _POOL[(n, F)]


def _render(gas, flags, n, F, T, publish_at, depth=None, draining=None):
    import torch

    from godot_audio_spatializer_amd import synth

    K = gas.capi
    srcs, psets = _inputs(n, F)
    hrir = synth.synthetic_hrir(np.random.default_rng(7), dirs=DIRS)
    ctx = gas.SpatializerContext(max_sources=n, frames=F, flags=flags)
    try:
        ctx.hrtf_load(hrir)
        if depth is not None:
            ctx.set_batch_depth(depth)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
        for e in (draining if draining is not None else ()):
            ctx.source_set_draining(int(slots[e]), True)
        ctx.params_publish_batch(slots, psets[0])
        d_srcs = [torch.from_numpy(s).cuda() for s in srcs]
        d_ps = [torch.from_numpy(p.view(np.uint8).reshape(n, -1).copy()).cuda() for p in psets[1:]]
        outs = torch.full((T, 1, F, 2), float("nan"), device="cuda")
        peaks = torch.zeros(T, n, 2, device="cuda")
        torch.cuda.synchronize()
        k = 0
        for t in range(T):
            if t in publish_at:
                ctx.params_publish_device(d_ps[k % len(d_ps)].data_ptr(), n)
                k += 1
            assert ctx.process_block_raw(d_srcs[t % len(d_srcs)].data_ptr(), slots if t == 0 else None, n, F, outs[t].data_ptr(), peaks[t].data_ptr(), K.MEM_DEVICE) == 0
        ctx.synchronize()
        return outs.cpu().numpy(), peaks.cpu().numpy()
    finally:
        ctx.close()


_BASE = {}


def _ordered(gas, F, n, pub, every_peak=False):
    key = (F, n, pub, every_peak)
    if key not in _BASE:
        K = gas.capi
        for k in [k for k in _BASE if k[:2] != (F, n)]:
            del _BASE[k]
        _BASE[key] = _render(gas, 0 if every_peak else K.FLAG_PEAKS_DRAINING_ONLY, n, F, T_ALL, PUBLISH[pub], draining=_draining(n))
    return _BASE[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"F{s[0]}_n{s[1]}")
@pytest.mark.parametrize("pub", list(PUBLISH))
@pytest.mark.parametrize("depth", [2, 16])
def test_batched_run_is_bitwise_the_ordered_mode(gas, shape, pub, depth):
    K = gas.capi
    F, n = shape
    base, pk0 = _ordered(gas, F, n, pub)
    got, pk1 = _render(gas, K.FLAG_PEAKS_DRAINING_ONLY | K.FLAG_PIPELINED_MIX | K.FLAG_BATCHED_LAUNCH, n, F, T_ALL, PUBLISH[pub], depth=depth, draining=_draining(n))
    assert not np.isnan(base).any() and np.abs(base).max() > 0
    d = _draining(n)
    assert np.isfinite(pk0[:, d]).all() and np.isposinf(np.delete(pk0, d, axis=1)).all()
    assert np.array_equal(base, got)
    assert np.array_equal(pk0, pk1)


@pytest.mark.parametrize("shape", [(512, 2051), (512, 14336), (256, 10240), (128, 6144)], ids=lambda s: f"F{s[0]}_n{s[1]}")
@pytest.mark.parametrize("depth", [2, 16])
def test_every_source_flagged(gas, shape, depth):
    """No GAS_FLAG_PEAKS_DRAINING_ONLY: every trip of every wave takes the exact-peak path."""
    K = gas.capi
    F, n = shape
    base, pk0 = _ordered(gas, F, n, "publish_inside_a_batch", every_peak=True)
    got, pk1 = _render(gas, K.FLAG_PIPELINED_MIX | K.FLAG_BATCHED_LAUNCH, n, F, T_ALL, PUBLISH["publish_inside_a_batch"], depth=depth, draining=_draining(n))
    assert not np.isnan(base).any() and np.isfinite(pk0).all()
    assert np.array_equal(base, got)
    assert np.array_equal(pk0, pk1)


@pytest.mark.parametrize("shape", [(512, 2051), (384, 2051), (256, 2051), (128, 128)], ids=lambda s: f"F{s[0]}_n{s[1]}")
def test_against_the_oracle(gas, ob, shape):
    """Depth 2 over five callbacks (two launches of two blocks, one callback left over), device-published rows taking
    effect at the second block of each launch, draining sources at the ends of waves: every mix within 1e-5 relative
    RMS of the oracle's, the draining sources' peaks within 2e-5 (tests/test_gpu_batched.py's bounds)."""
    import torch

    from godot_audio_spatializer_amd import synth
    from helpers import TOL, rel_rms

    K = gas.capi
    F, n = shape
    T = 5
    rng = np.random.default_rng(77 + F)
    hrir = synth.synthetic_hrir(np.random.default_rng(7), dirs=DIRS)
    draining = _draining(n)
    with gas.SpatializerContext(max_sources=n, frames=F, flags=K.FLAG_PEAKS_DRAINING_ONLY | K.FLAG_PIPELINED_MIX | K.FLAG_BATCHED_LAUNCH) as ctx:
        ctx.hrtf_load(hrir)
        ctx.set_batch_depth(2)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (K.FX_HRTF,))
        for e in draining:
            ctx.source_set_draining(int(slots[e]), True)
        params = synth.draw_params(rng, n, dirs=DIRS, frames=F)
        ctx.params_publish_batch(slots, params)
        ora = ob.BatchOracle(ob.KIND_EFFECT, n, F, chain=[K.FX_HRTF], hrir=hrir)
        outs = torch.full((T, 1, F, 2), float("nan"), device="cuda")
        peaks = torch.zeros(T, n, 2, device="cuda")
        keep, want, want_pk = [], [], []
        torch.cuda.synchronize()
        for t in range(T):
            if t in (1, 3):
                params = synth.draw_params(rng, n, dirs=DIRS, frames=F)
                d_p = torch.from_numpy(params.view(np.uint8).reshape(n, -1).copy()).cuda()
                keep.append(d_p)
                torch.cuda.synchronize()
                ctx.params_publish_device(d_p.data_ptr(), n)
            src = synth.draw_sources(rng, n, F)
            d_src = torch.from_numpy(src).cuda()
            keep.append(d_src)
            torch.cuda.synchronize()
            assert ctx.process_block_raw(d_src.data_ptr(), slots if t == 0 else None, n, F, outs[t].data_ptr(), peaks[t].data_ptr(), K.MEM_DEVICE) == 0
            _, rp, r64 = ora.block(params.astype(ob.PARAMS_DTYPE), src, want64=True)
            want.append(r64)
            want_pk.append(rp)
        ctx.synchronize()
        got, got_pk = outs.cpu().numpy(), peaks.cpu().numpy()
    for t in range(T):
        assert rel_rms(got[t][0], want[t][0]) <= TOL, f"callback {t}"
        np.testing.assert_allclose(got_pk[t][draining], want_pk[t][draining], rtol=2e-5, atol=1e-7, err_msg=f"callback {t}")
        assert np.all(np.isposinf(np.delete(got_pk[t], draining, axis=0)))
