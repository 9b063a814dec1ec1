"""HRTF callbacks past 8 sources per wave and past 256 partial rows: the sizes the README and bench.py quote, which no
other test looks at.  From 16 385 sources on a wave of k_hrtf_uni / k_hrtf_multi / k_hrtf_ols owns 9 to 64 sources (one
metadata lane each); from 131 073 on the grid leaves one residency round and a callback has more than 256 partial rows,
so the batched launch is refused, pending sums are "tall" (joined instead of carried) and k_mix_reduce runs its unrolled
trip more than once; from 196 608 on (or gas_tune_nt_hist_min) history rows are read and written non-temporally.

The reference is the same playbacks in callbacks of 1 024 (one source per wave, the regime the rest of the suite holds to
the oracle): a second context with the same slots, parameters and device source tensor (hrtf_large_ref.py).  Peaks of
plain-[HRTF] launches are bitwise those of the pieces for every playback and callback; mixes are additive over the
pieces to helpers.TOL; 136 entries at the seams of wave_range's split and at random go through the oracle alone.
Every case first asserts, from a restatement of the launch planning, that its shape still reaches its regime.

Figures, MI355X: worst over the callbacks of a case of rel_rms(mix, float64 sum of the piece mixes), TOL = 1e-5; every
plain-[HRTF] case had every peak bitwise that of the pieces, and so had both k_hrtf_ols forms.
  k_hrtf_uni, every peak     18 435 F=512 2.05e-7, F=384 2.03e-7; 131 067 2.24e-7 (contiguous and permuted);
                             131 073 2.53e-7; 393 293 2.36e-7
  k_hrtf_uni, draining only  131 067 2.48e-7; 393 293 2.61e-7
  two buses, 131 067         2.11e-7 (the worse of the two buses)
  k_hrtf_ols, 131 067        cross-fade + draining only 2.01e-7, [ER, HRTF] 2.18e-7; peaks bitwise in both
  [HIGHSHELF, HRTF]          18 435 F=256 3.09e-7; 32 767 2.09e-7 (peaks bitwise); 131 067 1.85e-7 (serial filter stage on
                             both sides, peaks bitwise: see test_filter_in_front)
The same figure at three sizes, k_hrtf_uni with every peak: 2.05e-7 at 18 435, 2.24e-7 at 131 067,
2.36e-7 at 393 293 sources -- the f32 sum does not deepen measurably.  Anchor entries against the oracle: at most 6.3e-7
relative for plain [HRTF] (bar 2e-5), 2.2e-5 behind a filter (bar 1e-4).
"""
import numpy as np
import pytest

import hrtf_large_ref as R
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

HRTF, ER, HS = R.HRTF, R.ER, R.HIGHSHELF

# n -> (workgroups, most sources per wave, fewest): the regime each shape was chosen for
REGIME = {
    18435: (256, 10, 9),  # first step past 8 per wave
    32767: (256, 16, 15),  # the largest callback whose [filter, HRTF] chain runs in one launch (k_hrtf_uni<FLT>)
    131067: (256, 64, 63),  # every metadata lane, 2 043 waves of 64; still one round, still batchable
    131073: (257, 64, 63),  # first grid past one round: 257 partial rows
    393293: (769, 64, 63),  # three rounds: the reduce's four-row trip three times plus a tail
}


@pytest.fixture(autouse=True)
def _default_launch_forms(monkeypatch):
    for name in ("GAS_UNI_ER", "GAS_UNI_FLT", "GAS_SHELF_SCAN", "GAS_XCD_ORDER_AUTO_MIN", "GAS_UNI12_MIN", "GAS_NT_HIST_MIN"):
        monkeypatch.delenv(name, raising=False)


# ------------------------------------------------------------------------------ 1, 3. k_hrtf_uni, every peak; slot addressing
UNI_SHAPES = [(18435, 512, False), (18435, 384, False), (131067, 128, False), (131067, 128, True), (131073, 128, False), (393293, 128, False)]


@pytest.mark.parametrize("n,F,permuted", UNI_SHAPES, ids=[f"{n}-F{F}-{'permuted' if p else 'contiguous'}" for n, F, p in UNI_SHAPES])
def test_uni_every_peak_is_the_peak_in_callbacks_of_1024(gas, ob, n, F, permuted):
    """flags = 0: every playback reports its exact peak.  131 067 runs twice: with the list in allocation order (the
    contiguous form, g.slots == nullptr in the kernel) and with a permuted slot list."""
    R.run_against_pieces(gas, ob, n=n, F=F, blocks=6 if F == 128 else 4, permuted=permuted, want_regime=REGIME[n], want_kernel="k_hrtf_uni", seed=n % 97 + F, label=f"uni n={n} F={F}{' permuted' if permuted else ''}")


# ------------------------------------------------------------------------------------------- 2. k_hrtf_uni, draining only
@pytest.mark.parametrize("n", [131067, 393293])
def test_uni_draining_only(gas, ob, n):
    """GAS_FLAG_PEAKS_DRAINING_ONLY, every 11th playback (and the anchor entries) draining: the peak bitmap is indexed
    (e + peak_bit_base) >> 5 with e up to n, where the pieces index it below 1 024."""
    R.run_against_pieces(gas, ob, n=n, F=128, flags=gas.capi.FLAG_PEAKS_DRAINING_ONLY, draining_every=11, want_regime=REGIME[n], want_kernel="k_hrtf_uni", seed=11, label=f"uni draining n={n}")


# --------------------------------------------------------------------------------------------------------- 8. two buses
def test_two_buses_64_sources_per_wave(gas, ob):
    """[HRTF] playbacks on two buses with random sends (k_hrtf_uni<BUS2>): per-lane route weights broadcast like the
    rest of the metadata, bus 1's LDS sums touched by 64 sources per wave."""
    R.run_against_pieces(gas, ob, n=131067, F=128, buses=2, want_regime=REGIME[131067], seed=8, label="two buses n=131067")


# ------------------------------------------------------------------------------------------------ 9. the k_hrtf_ols forms
def test_ols_crossfade_draining_only(gas, ob):
    """Plain [HRTF] under GAS_FLAG_HRTF_CROSSFADE | GAS_FLAG_PEAKS_DRAINING_ONLY, every 7th playback draining: 112 343
    frequency-domain sources outgrow their 191 workgroups of the round (`need` overrides `share`: 220 workgroups, 63 and
    64 per wave); the 18 724 exact-peak sources fill their share (65 workgroups, 36 and 37 per wave -- an exact-peak group
    cannot outgrow its share at this n: that would take n_fd + 2 n_pk > 262 144).  285 partial rows."""
    K = gas.capi
    want = dict(fd=(220, 64, 63), pk=(65, 37, 36))
    res = R.run_against_pieces(gas, ob, n=131067, F=128, flags=K.FLAG_HRTF_CROSSFADE | K.FLAG_PEAKS_DRAINING_ONLY, draining_every=7, plan="ols", want_regime=want, want_kernel="k_hrtf_ols", peak_bar=(2e-5, 1e-7), seed=9, label="ols crossfade n=131067")
    assert res["rows"] == 285


def test_ols_er_hrtf(gas, ob):
    """[ER, HRTF] with every peak on the smallest ring the chain accepts at F = 128 (256 frames): all playbacks in the
    exact-peak group of k_hrtf_ols<ER>, 256 workgroups, 63 and 64 per wave."""
    want = dict(pk=(256, 64, 63))
    R.run_against_pieces(gas, ob, n=131067, F=128, chain=(ER, HRTF), ring=256, plan="ols", want_regime=want, want_kernel="k_hrtf_ols<ER>", peak_bar=(2e-5, 1e-7), seed=10, label="ols [ER, HRTF] n=131067")


# ----------------------------------------------------------------------------------------------------- 10. filter in front
@pytest.mark.parametrize("n,F", [(18435, 256), (32767, 128), (131067, 128)])
def test_filter_in_front(gas, ob, n, F, monkeypatch):
    """[HIGHSHELF, HRTF], every 97th shelf at 60 Hz (the serial two-lane path inside a wave of several sources).  Peaks
    against the pieces and against the oracle at the bar test_filter_stage_as_a_scan_matches_oracle gives scan-form
    peaks, rtol 1e-4 / atol 1e-6.

    The one-launch form k_hrtf_uni<FLT> is taken where k_shelf_scan would be (gas_shelf_scan_applies: 512 <= n <
    32 768), so its per-wave coefficient table flt_all[wave][64][13] never holds more than 16 sources: 18 435 (9 and 10
    per wave) and 32 767 (15 and 16, the most the form can meet) run it, and so do their pieces of 1 024.

    At 131 067 the filter is the serial stage kernel (the engine's order) with k_hrtf_uni over its rows behind it, 63
    and 64 per wave.  Pieces of 1 024 would by default run the scan form, another arithmetic; the comparison is between
    the same playbacks in the same arithmetic, so this case runs under GAS_SHELF_SCAN=0, which leaves the callback of
    131 067 as it is and sends the pieces down the serial road too.  Every operation on a source is then the same on
    both sides, and the peaks are asserted bitwise, which is more than the bar.

    Across the two forms the bar cannot hold at this population, whichever code is right (measured, MI355X: 59 and 67
    of 131 067 playbacks outside rtol 1e-4 in callbacks 3 and 5, worst 11.0 times the band, the callback of 131 067
    within 0.16 of the band of the oracle).  The playbacks outside are shelves both low and deep, 800 to 1 150 Hz at
    gain 0.085 to 0.10: all-pole peak gain 480 to 1 270 (shelf_scan_ref.allpole_peak_gain), which the gate sends serial
    in both forms.  They were scanned under their previous coefficients; the last-bit difference the scan leaves in
    y[-1], y[-2] is amplified by that gain once the coefficients snap, and shows against the small settled output one
    callback later.  DESIGN.md 3.1 has the figures."""
    if n >= 32768:
        monkeypatch.setenv("GAS_SHELF_SCAN", "0")
    res = R.run_against_pieces(gas, ob, n=n, F=F, chain=(HS, HRTF), blocks=6 if F == 128 else 4, want_regime=REGIME[n], want_kernel="staged effect chain", peak_bar=(1e-4, 1e-6), anchor_bar=(1e-4, 1e-6), shelf_cutoffs=True, seed=n % 89, label=f"[HIGHSHELF, HRTF] n={n} F={F}")
    if n >= 32768:
        assert res["peaks_bitwise"], "the serial filter stage and k_hrtf_uni over its rows: a playback's peak depends on the size of the callback"


# ------------------------------------------------------------------------------- 4, 5. k_hrtf_multi at its limit; refused
def _render_batched(gas, flags, n, F, srcs, first, rows, draining, depth=None):
    """Six device-memory callbacks with the list unchanged, a device parameter row published before callbacks 2 and 3;
    then three more under the profiler.  -> (mixes [6][1][F][2], peaks [6][n][2], profile of the last three)."""
    import torch

    K = gas.capi
    T = len(srcs)
    ctx = gas.SpatializerContext(max_sources=n, frames=F, flags=flags)
    try:
        ctx.hrtf_load(R.hrir())
        if depth is not None:
            ctx.set_batch_depth(depth)
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (HRTF,))
        for s in slots[draining]:
            ctx.source_set_draining(int(s), True)
        ctx.params_publish_batch(slots, first)
        outs = torch.full((T + 3, 1, F, 2), float("nan"), device="cuda")
        peaks = torch.full((T + 3, n, 2), float("nan"), device="cuda")
        torch.cuda.synchronize()
        for t in range(T):
            if t in rows:
                ctx.params_publish_device(rows[t].data_ptr(), n)
            assert ctx.process_block_raw(srcs[t].data_ptr(), slots if t == 0 else None, n, F, outs[t].data_ptr(), peaks[t].data_ptr(), K.MEM_DEVICE) == 0
        ctx.synchronize()
        ctx.profile_enable(1)
        ctx.profile_read(reset=True)
        for t in range(3):
            assert ctx.process_block_raw(srcs[t].data_ptr(), None, n, F, outs[T + t].data_ptr(), peaks[T + t].data_ptr(), K.MEM_DEVICE) == 0
        ctx.synchronize()
        prof = ctx.profile_read()
        ctx.profile_enable(0)
        return outs, peaks, prof
    finally:
        ctx.close()


@pytest.mark.parametrize("n,kernel,launches", [(131067, "k_hrtf_multi", 1), (131073, "k_hrtf_uni", 3)], ids=["131067-batched", "131073-refused"])
def test_batched_launch_at_its_limit_and_refused(gas, ob, n, kernel, launches):
    """GAS_FLAG_PEAKS_DRAINING_ONLY | GAS_FLAG_PIPELINED_MIX | GAS_FLAG_BATCHED_LAUNCH at depth 3 against the ordered
    mode, bitwise (the contract of test_gpu_batched.py).  131 067: the largest callback batchable() accepts -- 256
    workgroups, 64 sources per wave, k_hrtf_multi's history through memory.  131 073: 257 workgroups, the batch is
    refused, every pending sum is tall (run_groups joins instead of handing it to a carrier) and the profiled kernel is
    k_hrtf_uni.  The ordered mode's draining anchor entries go through the oracle."""
    import torch

    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F, T = 128, 6
    wgs = R.uni_partials(n)
    R.assert_regime(n, wgs, REGIME[n], f"batched n={n}")
    assert (wgs <= R.ROUND) == (kernel == "k_hrtf_multi"), "batchable()'s limit of 256 workgroups moved"
    rng = np.random.default_rng(45)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(45 + n)
    srcs = [R.device_sources(gen, n, F) for _ in range(T)]
    params = {t: synth.draw_params(rng, n, dirs=R.DIRS, frames=F) for t in (0, 2, 3)}
    rows = {t: torch.from_numpy(params[t].view(np.uint8).reshape(n, -1).copy()).cuda() for t in (2, 3)}
    torch.cuda.synchronize()
    # every 11th playback drains, and so do the oracle's entries: those at the seams of the split and 128 random ones
    anchor = R.pick_anchor(np.arange(n), wgs, 4)
    draining = np.union1d(np.arange(0, n, 11), anchor)
    base, pk0, prof0 = _render_batched(gas, K.FLAG_PEAKS_DRAINING_ONLY, n, F, srcs, params[0], rows, draining)
    got, pk1, prof1 = _render_batched(gas, K.FLAG_PEAKS_DRAINING_ONLY | K.FLAG_PIPELINED_MIX | K.FLAG_BATCHED_LAUNCH, n, F, srcs, params[0], rows, draining, depth=3)
    assert not bool(torch.isnan(base).any()) and float(base.abs().max()) > 0
    assert bool(torch.equal(R.bits(base), R.bits(got))), "mixes differ from the ordered mode"
    assert bool(torch.equal(R.bits(pk0), R.bits(pk1))), "peaks differ from the ordered mode"
    assert prof0["kernel"].startswith("k_hrtf_uni") and prof0["launches"] == 3
    assert prof1["kernel"].startswith(kernel) and prof1["launches"] == launches, prof1
    # the ordered mode against the oracle
    ora = ob.BatchOracle(ob.KIND_EFFECT, len(anchor), F, chain=[HRTF], hrir=R.hrir())
    d_anchor = torch.from_numpy(anchor.astype(np.int64)).cuda()
    p = params[0]
    for t in range(T):
        p = params.get(t, p)
        _, rp, _ = ora.block(p[anchor].astype(ob.PARAMS_DTYPE), srcs[t][d_anchor].cpu().numpy())
        np.testing.assert_allclose(pk0[t][d_anchor].cpu().numpy(), rp, rtol=2e-5, atol=1e-7, err_msg=f"callback {t}")
    rest = np.ones(n, bool)
    rest[draining] = False
    assert bool(torch.isposinf(pk0[:T][:, torch.from_numpy(rest).cuda()]).all())


# ------------------------------------------------------------------------------------ 6. tall pending sums at small size
def _render_tall(gas, flags, F, n_h, n_s, srcs, params, depth=None):
    import torch

    K = gas.capi
    T = len(srcs)
    n = n_h + n_s
    ctx = gas.SpatializerContext(max_sources=n, frames=F, flags=flags)
    try:
        ctx.hrtf_load(R.hrir())
        if depth is not None:
            ctx.set_batch_depth(depth)
        both = np.concatenate([ctx.source_alloc_many(n_h, K.KIND_EFFECT, (HRTF,)), ctx.source_alloc_many(n_s, K.KIND_EFFECT, (HS,))])
        for s in both[:n_h:11]:
            ctx.source_set_draining(int(s), True)
        outs = torch.full((T, 1, F, 2), float("nan"), device="cuda")
        peaks = torch.zeros((T, n, 2), device="cuda")
        torch.cuda.synchronize()
        for t in range(T):
            m = n if t < 3 else n_h  # callbacks 0 to 2: the mixed list; from 3 on: the [HRTF] entries alone
            if t in params:
                ctx.params_publish_batch(both, params[t])
            if t == 6:
                ctx.join_outputs()
            assert ctx.process_block_raw(srcs[t].data_ptr(), both[:m] if t in (0, 3) else None, m, F, outs[t].data_ptr(), peaks[t].data_ptr(), K.MEM_DEVICE) == 0
        ctx.synchronize()
        return outs, peaks
    finally:
        ctx.close()


def test_tall_pending_sums_at_small_size(gas, ob):
    """2 048 [HRTF] playbacks (256 partial rows) plus 64 [HIGHSHELF] playbacks in one list: more than 256 rows, so the
    pending sum of such a callback is tall.  Under GAS_FLAG_PIPELINED_MIX the next carrier launch must join instead of
    carrying it (run_groups: `fits`); with GAS_FLAG_BATCHED_LAUNCH at depth 3 callbacks 3 to 5 form the first batch
    while callback 2's tall sum is still pending (run_hrtf_batch: `tall`).  A join_outputs before callback 6.  Every
    callback bitwise the ordered mode, which is itself held to the oracle at callbacks 0 and 3."""
    import torch

    from godot_audio_spatializer_amd import synth

    K = gas.capi
    F, n_h, n_s, T = 256, 2048, 64, 8
    n = n_h + n_s
    assert R.regime(n_h, R.uni_partials(n_h)) == (256, 1, 1), "2 048 [HRTF] playbacks no longer write 256 partial rows"
    rng = np.random.default_rng(6)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(6)
    srcs = [R.device_sources(gen, n if t < 3 else n_h, F) for t in range(T)]
    params = {t: synth.draw_params(rng, n, dirs=R.DIRS, frames=F) for t in (0, 2, 6)}
    torch.cuda.synchronize()
    base, pk0 = _render_tall(gas, K.FLAG_PEAKS_DRAINING_ONLY, F, n_h, n_s, srcs, params)
    assert not bool(torch.isnan(base).any()) and float(base.abs().max()) > 0
    for name, flags, depth in (("pipelined", K.FLAG_PIPELINED_MIX, None), ("batched", K.FLAG_PIPELINED_MIX | K.FLAG_BATCHED_LAUNCH, 3)):
        got, pk1 = _render_tall(gas, K.FLAG_PEAKS_DRAINING_ONLY | flags, F, n_h, n_s, srcs, params, depth)
        diff = [t for t in range(T) if not torch.equal(R.bits(base[t]), R.bits(got[t]))]
        assert not diff, f"{name}: mixes of callbacks {diff} differ from the ordered mode"
        assert bool(torch.equal(R.bits(pk0), R.bits(pk1))), f"{name}: peaks differ from the ordered mode"
    ora_h = ob.BatchOracle(ob.KIND_EFFECT, n_h, F, chain=[HRTF], hrir=R.hrir())
    ora_s = ob.BatchOracle(ob.KIND_EFFECT, n_s, F, chain=[HS])
    p = params[0]
    for t in range(4):
        p = params.get(t, p)
        src = srcs[t].cpu().numpy()
        _, _, want = ora_h.block(p[:n_h].astype(ob.PARAMS_DTYPE), src[:n_h], want64=True)
        if t < 3:
            want = want + ora_s.block(p[n_h:].astype(ob.PARAMS_DTYPE), src[n_h:], want64=True)[2]
        if t in (0, 3):
            e = rel_rms(base[t, 0].cpu().numpy(), want[0])
            print(f"tall sums: ordered mode against the oracle, callback {t}: {e:.3e}")
            assert e <= TOL, f"callback {t}: {e}"


# ------------------------------------------------------------------------------------------- 7. non-temporal history rows
@pytest.fixture()
def nt_hist(gas):
    """gas_tune_nt_hist_min is process-global: hand out the setter, restore the value found."""
    lib = gas.load_library()
    was = lib.gas_tune_nt_hist_min(0xFFFFFFFF)
    lib.gas_tune_nt_hist_min(was)
    yield lib, was
    lib.gas_tune_nt_hist_min(was)


def _run_plain(gas, n, F, blocks, seed, keep_host=False):
    """`blocks` host-published parameter sets and device sources through one plain-[HRTF] context, every peak."""
    import torch

    from godot_audio_spatializer_amd import synth

    K = gas.capi
    rng = np.random.default_rng(seed)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    outs = torch.full((blocks, 1, F, 2), float("nan"), device="cuda")
    peaks = torch.full((blocks, n, 2), float("nan"), device="cuda")
    host = []
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        ctx.hrtf_load(R.hrir())
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, (HRTF,))
        for t in range(blocks):
            p = synth.draw_params(rng, n, dirs=R.DIRS, frames=F)
            ctx.params_publish_batch(slots, p)
            src = R.device_sources(gen, n, F)
            torch.cuda.synchronize()
            assert ctx.process_block_raw(src.data_ptr(), slots if t == 0 else None, n, F, outs[t].data_ptr(), peaks[t].data_ptr(), K.MEM_DEVICE) == 0
            ctx.synchronize()
            if keep_host:
                host.append((p, src.cpu().numpy()))
    return outs, peaks, host


@pytest.mark.parametrize("n,F", [(2051, 512), (18435, 512), (2051, 256)])
def test_non_temporal_history_rows(gas, ob, nt_hist, n, F):
    """nt_hist: history rows written non-temporally by callback t and read back non-temporally by callback t + 1 (on
    from 196 608 sources; here through gas_tune_nt_hist_min(1)).  Only the cache policy differs, so five callbacks with
    changing parameters are bitwise those of the default; at 2 051 sources the non-temporal run is held to the oracle.
    F = 256: HQ = 6 is no multiple of 4, the flag must change nothing at all."""
    lib, default = nt_hist
    assert default > 18435, f"non-temporal history rows now start at {default} sources: the default run of this test would take them too"
    assert lib.gas_tune_nt_hist_min(1) == default
    nt, pk_nt, host = _run_plain(gas, n, F, 5, seed=70 + F, keep_host=(n == 2051 and F == 512))
    assert lib.gas_tune_nt_hist_min(default) == 1
    plain, pk_plain, _ = _run_plain(gas, n, F, 5, seed=70 + F)
    import torch

    assert not bool(torch.isnan(nt).any()) and float(nt.abs().max()) > 0
    assert bool(torch.equal(R.bits(nt), R.bits(plain))), "mixes differ between non-temporal and default history rows"
    assert bool(torch.equal(R.bits(pk_nt), R.bits(pk_plain))), "peaks differ between non-temporal and default history rows"
    if host:
        ora = ob.BatchOracle(ob.KIND_EFFECT, n, F, chain=[HRTF], hrir=R.hrir())
        for t, (p, src) in enumerate(host):
            _, rp, r64 = ora.block(p.astype(ob.PARAMS_DTYPE), src, want64=True)
            e = rel_rms(nt[t, 0].cpu().numpy(), r64[0])
            print(f"non-temporal history rows n={n} F={F} callback {t}: against the oracle {e:.3e}")
            assert e <= TOL, f"callback {t}: {e}"
            np.testing.assert_allclose(pk_nt[t].cpu().numpy(), rp, rtol=2e-5, atol=1e-7, err_msg=f"callback {t}")
