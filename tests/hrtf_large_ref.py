"""Helpers of tests/test_gpu_hrtf_large_callbacks.py: a Python restatement of the HRTF launch planning, and the runner that
holds one callback over n list entries (context A) to the same playbacks in callbacks of 1 024 (context B).

The planning restated here is gas_hrtf_uni_partials (csrc/k_hrtf_uni.hip), gas_hrtf_plan (csrc/k_hrtf_ols.hip) and
wave_range (csrc/gas_hrtf_wave.h).  The tests assert with it that a shape still reaches the regime it was chosen for, and
take from it the list entries at the seams of the split; if the planning changes, they fail with that message."""
import ctypes as C

import numpy as np

from helpers import TOL, rel_rms

PIECE = 1024  # one source per wave on 128 workgroups: the regime the rest of the suite holds to the oracle
WAVES = 8  # waves per workgroup of k_hrtf_uni (eight-wave form), k_hrtf_multi and k_hrtf_ols
ROUND = 256  # workgroups resident at once (one per CU)
DIRS = 64
HRTF, ER, HIGHSHELF = 3, 2, 1


def _wgs_for(n, cap):
    """At least one source per wave, at most `cap` workgroups unless a wave would then own more than 64 sources."""
    want, need = -(-n // WAVES), -(-n // (WAVES * 64))
    return max(min(want, cap), need)


def uni_partials(n):
    """gas_hrtf_uni_partials: workgroups (= partial rows) of a k_hrtf_uni / k_hrtf_multi launch over n sources."""
    return _wgs_for(n, ROUND)


def ols_plan(n_fd, n_pk, pk_weight=2):
    """gas_hrtf_plan: (workgroups of the frequency-domain group, of the exact-peak group, the frequency-domain group's
    share of the round) of one k_hrtf_ols launch."""
    budget = ROUND * 4 * 2 // WAVES  # GAS_HRTF_WAVES_PER_SIMD = 2
    wgs_pk, budget_fd = 0, budget
    if n_pk:
        share = -(-(budget * pk_weight * n_pk) // (n_fd + pk_weight * n_pk)) if n_fd else budget
        share = max(1, min(share, budget - (1 if n_fd else 0)))
        wgs_pk = _wgs_for(n_pk, share)
        budget_fd = budget - wgs_pk if budget > wgs_pk else 1
    return (_wgs_for(n_fd, budget_fd) if n_fd else 0), wgs_pk, budget_fd


def wave_range(n, gw, n_waves):
    """wave_range: sources [first, last) of wave gw out of n_waves (the first n % n_waves waves take one more)."""
    base, rem = divmod(n, n_waves)
    first = gw * base + min(gw, rem)
    return first, first + base + (1 if gw < rem else 0)


def regime(n, wgs):
    """(workgroups, most sources a wave owns, fewest) of n sources split over wgs workgroups."""
    base, rem = divmod(n, wgs * WAVES)
    return wgs, base + (1 if rem else 0), base


def seam_entries(n, wgs):
    """Group-local entries at the seams of the split: first and last entry of wave 0, of the last wave that takes one
    extra source, of the first wave that does not, and entry n - 1."""
    n_waves = wgs * WAVES
    rem = n % n_waves
    waves = {0, n_waves - 1}
    if rem:
        waves |= {rem - 1, rem}
    out = {n - 1}
    for gw in waves:
        first, last = wave_range(n, gw, n_waves)
        if last > first:
            out |= {first, last - 1}
    return sorted(out)


def where_in_launch(k, n, wgs):
    """(workgroup, wave, lane) of group-local entry k, for failure messages."""
    n_waves = wgs * WAVES
    base, rem = divmod(n, n_waves)
    gw = k // (base + 1) if k < rem * (base + 1) else rem + (k - rem * (base + 1)) // max(base, 1)
    return gw // WAVES, gw % WAVES, k - wave_range(n, gw, n_waves)[0]


def assert_regime(n, wgs, want, what):
    got = regime(n, wgs)
    assert got == want, f"{what}: the launch planning changed -- {n} sources now run on {got[0]} workgroups with {got[2]} to {got[1]} sources per wave, this case was built for {want[0]} workgroups with {want[2]} to {want[1]}"


_HRIR = {}


def hrir(dirs=DIRS):
    from godot_audio_spatializer_amd import synth

    if dirs not in _HRIR:
        _HRIR[dirs] = synth.synthetic_hrir(np.random.default_rng(7), dirs=dirs)
    return _HRIR[dirs]


def device_sources(gen, n, F):
    """uniform(-0.5, 0.5) float32 [n][F][2], drawn on the device."""
    import torch

    return torch.rand((n, F, 2), generator=gen, device="cuda", dtype=torch.float32) - 0.5


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def call(ctx, src_ptr, slots, n, F, out_ptr, peaks_ptr, buses=0):
    """gas_process_block, or gas_process_block_buses (its raw form) for buses > 0, over device memory -> status."""
    K = ctx.lib
    if not buses:
        return ctx.process_block_raw(src_ptr, slots, n, F, out_ptr, peaks_ptr, 1)
    s = np.ascontiguousarray(slots, dtype=np.uint32) if slots is not None else None
    sp = s.ctypes.data_as(C.c_void_p) if s is not None else None
    return K.gas_process_block_buses(ctx.h, C.c_void_p(src_ptr), sp, n, F, C.c_void_p(out_ptr), buses, C.c_void_p(peaks_ptr), 1)


def pick_anchor(peak_entries, wgs, seed):
    """List entries for the oracle anchor: those at the seams of the peak-reporting group's split (peak_entries: its
    list entries in launch order, wgs: its workgroups) plus 128 (or more, up to 136 in all) random ones of that group."""
    m = len(peak_entries)
    seams = seam_entries(m, wgs)
    rest = np.setdiff1d(np.arange(m), seams)
    more = np.random.default_rng(seed).choice(rest, max(128, 136 - len(seams)), replace=False)  # (seams coincide where a wave owns one source, or the last wave with an extra source is the last but one)
    local = np.sort(np.concatenate([np.asarray(seams, dtype=np.int64), more]))
    assert len(local) >= 136
    return np.asarray(peak_entries)[local]


def run_against_pieces(gas, ob, *, n, F, chain=(HRTF,), flags=0, blocks=6, permuted=False, draining_every=0, ring=0, buses=0, plan="uni", want_regime=None, want_kernel=None, peak_bar=None, anchor_bar=(2e-5, 1e-7), shelf_cutoffs=False, seed=0, label=""):
    """Context A runs `blocks` callbacks over all n list entries; context B has the same slots, parameters and device
    source tensor and runs each callback as ceil(n / 1024) calls over consecutive pieces of the list.

    Asserted per callback: every playback's peak in A against B (bitwise, or within peak_bar = (rtol, atol)), +inf for
    the playbacks that report none, rel_rms(A's mix, float64 sum of B's piece mixes) <= TOL per bus, and A's peaks of
    the anchor entries against ob.BatchOracle within anchor_bar.  -> dict(worst_mix, peaks_bitwise, worst_anchor)."""
    import torch

    from godot_audio_spatializer_amd import synth

    K = gas.capi
    rng = np.random.default_rng(1000 + seed)
    h = hrir()
    pieces = -(-n // PIECE)
    crossfade = bool(flags & K.FLAG_HRTF_CROSSFADE)
    draining_only = bool(flags & K.FLAG_PEAKS_DRAINING_ONLY)

    # ---- which entries report a peak, how the launch splits them, which of them the oracle sees
    exact = np.ones(n, bool)
    if draining_only:
        exact[:] = False
        exact[::draining_every] = True
    if plan == "uni":  # one group in list order: k_hrtf_uni over every entry, peaks chosen by the bitmap
        wgs = uni_partials(n)
        peak_entries = np.arange(n)
        anchor = pick_anchor(peak_entries, wgs, seed)
        exact[anchor] = True  # draining only: the seams are seams of the whole list, so they (and the random picks) drain as well
        assert_regime(n, wgs, want_regime, label)
        assert regime(min(n, PIECE), uni_partials(min(n, PIECE))) == (PIECE // WAVES, 1, 1), "a piece of 1 024 no longer runs one source per wave"
        n_rows = wgs
    else:  # k_hrtf_ols: the frequency-domain group, then the exact-peak group behind it, each split on its own
        n_pk = int(exact.sum())
        wgs_fd, wgs_pk, budget_fd = ols_plan(n - n_pk, n_pk)
        if n - n_pk:
            assert_regime(n - n_pk, wgs_fd, want_regime["fd"], label + " (frequency-domain group)")
            assert -(-(n - n_pk) // (WAVES * 64)) > budget_fd, f"{label}: the frequency-domain group no longer outgrows its share of the round"
        assert_regime(n_pk, wgs_pk, want_regime["pk"], label + " (exact-peak group)")
        peak_entries = np.flatnonzero(exact)
        anchor = pick_anchor(peak_entries, wgs_pk, seed)
        n_rows = wgs_fd + wgs_pk
    assert exact[anchor].all() and len(anchor) >= 136

    ctxs = [gas.SpatializerContext(max_sources=n, frames=F, er_ring_frames=ring, flags=flags) for _ in range(2)]
    try:
        lists = []
        for ctx in ctxs:
            ctx.hrtf_load(h)
            slots = ctx.source_alloc_many(n, K.KIND_EFFECT, chain)
            assert np.array_equal(slots, slots[0] + np.arange(n, dtype=np.uint32)), "slots are no longer handed out in ascending order: the contiguous form is not reached"
            lists.append(slots)
        assert np.array_equal(lists[0], lists[1])
        lst = lists[0]
        if permuted:
            lst = lst[np.random.default_rng(2000 + seed).permutation(n)]
        if draining_only:
            for ctx in ctxs:
                for s in lst[exact]:
                    ctx.source_set_draining(int(s), True)
        A, B = ctxs
        ora = ob.BatchOracle(ob.KIND_EFFECT, len(anchor), F, chain=list(chain), hrir=h, er_ring_frames=max(ring, 1), crossfade=crossfade)
        nb = max(buses, 1)
        out_a = torch.full((nb, 1, F, 2), float("nan"), device="cuda")
        out_b = torch.full((pieces, nb, 1, F, 2), float("nan"), device="cuda")
        pk_a = torch.full((n, 2), float("nan"), device="cuda")
        pk_b = torch.full((n, 2), float("nan"), device="cuda")
        d_exact = torch.from_numpy(exact).cuda()
        d_anchor = torch.from_numpy(anchor.astype(np.int64)).cuda()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(3000 + seed)
        A.profile_enable(1)
        A.profile_read(reset=True)
        res = dict(worst_mix=0.0, peaks_bitwise=True, worst_anchor=0.0, worst_peak=0.0)
        outside = []
        for t in range(blocks):
            if t % 2 == 0:  # gain ramps and direction switches at every second callback
                p = synth.draw_params(rng, n, dirs=DIRS, ring_frames=max(ring, 2 * F), frames=F)
                if shelf_cutoffs:  # as test_filter_stage_as_a_scan_matches_oracle draws them: every 97th next to the unit circle (the serial two-lane path)
                    p["fx_shelf_cutoff_hz"] = np.exp(rng.uniform(np.log(800.0), np.log(12000.0), n)).astype(np.float32)
                    p["fx_shelf_cutoff_hz"][::97] = 60.0
                if buses:
                    routes = K.bus_routes(n)
                    routes["dry_bus"] = rng.integers(0, buses, n)
                    routes["send_bus"] = np.where(rng.uniform(size=n) < 0.6, rng.integers(0, buses, n), K.BUS_NONE)
                    routes["send"][:, 0, :] = rng.uniform(0.0, 1.0, (n, 2))
                for ctx in ctxs:
                    ctx.params_publish_batch(lst, p)
                    if buses:
                        ctx.bus_routes_publish(lst, routes)
            src = device_sources(gen, n, F)
            torch.cuda.synchronize()
            rc = call(A, src.data_ptr(), lst if t == 0 else None, n, F, out_a.data_ptr(), pk_a.data_ptr(), buses)
            assert rc == 0, f"{label} callback {t}: context A: status {rc}"
            for j in range(pieces):
                off = j * PIECE
                m = min(PIECE, n - off)
                rc = call(B, src.data_ptr() + off * F * 8, lst[off:off + m], m, F, out_b[j].data_ptr(), pk_b.data_ptr() + off * 8, buses)
                assert rc == 0, f"{label} callback {t} piece {j}: context B: status {rc}"
            A.synchronize()
            B.synchronize()
            # ---- peaks: every entry, none left out
            same = bool(torch.equal(bits(pk_a), bits(pk_b)))
            res["peaks_bitwise"] = res["peaks_bitwise"] and same
            if not same:
                bad = torch.nonzero((bits(pk_a) != bits(pk_b)).any(dim=1)).flatten().cpu().numpy()
                first = [(int(k), where_in_launch(int(k), n, uni_partials(n))) for k in bad[:6]] if plan == "uni" else [int(k) for k in bad[:6]]
                msg = f"{label} callback {t}: {len(bad)} of {n} playbacks report another peak than in callbacks of {PIECE}; first entries (entry, (workgroup, wave, lane)): {first}"
                assert peak_bar is not None, msg
                fa, fb = pk_a[d_exact].cpu().numpy(), pk_b[d_exact].cpu().numpy()
                dev = np.abs(fa - fb) / (peak_bar[1] / peak_bar[0] + np.abs(fb))
                res["worst_peak"] = max(res["worst_peak"], float(dev.max()))
                if dev.max() > peak_bar[0]:  # reported after the last callback, so that every figure of the case is printed first
                    out = int((dev > peak_bar[0]).any(axis=1).sum())
                    outside.append(f"{msg}; {out} of them outside rtol {peak_bar[0]:.0e} / atol {peak_bar[1]:.0e}, worst {dev.max() / peak_bar[0]:.2f} of the band")
            assert bool(torch.isfinite(pk_a[d_exact]).all()), f"{label} callback {t}: a playback that reports its peak has none"
            if not exact.all():
                assert bool(torch.isposinf(pk_a[~d_exact]).all()) and bool(torch.isposinf(pk_b[~d_exact]).all()), f"{label} callback {t}: a playback that is not draining reports something other than +inf"
            # ---- mix: additive over the pieces
            mix_a = out_a.cpu().numpy().astype(np.float64)
            sum_b = out_b.double().sum(dim=0).cpu().numpy()
            for b in range(nb):
                e = rel_rms(mix_a[b, 0], sum_b[b, 0])
                res["worst_mix"] = max(res["worst_mix"], float(e))
                print(f"{label} callback {t} bus {b}: rel_rms(mix of {n}, sum of {pieces} piece mixes) = {e:.3e}")
                assert np.isfinite(mix_a[b]).all() and np.abs(mix_a[b]).max() > 0
                assert e <= TOL, f"{label} callback {t} bus {b}: {e}"
            # ---- the oracle on the anchor entries alone
            _, rp, _ = ora.block(p[anchor].astype(ob.PARAMS_DTYPE), src[d_anchor].cpu().numpy())
            got = pk_a[d_anchor].cpu().numpy()
            dev = np.abs(got - rp) / (anchor_bar[1] / anchor_bar[0] + np.abs(rp))
            res["worst_anchor"] = max(res["worst_anchor"], float(dev.max()))
            np.testing.assert_allclose(got, rp, rtol=anchor_bar[0], atol=anchor_bar[1], err_msg=f"{label} callback {t}: anchor entries {anchor[:8]}... against the oracle")
            del src
        prof = A.profile_read()
        A.profile_enable(0)
        if want_kernel is not None:
            assert prof["kernel"].startswith(want_kernel), f"{label}: the callback ran {prof['kernel']!r}, this case is about {want_kernel!r}"
        res["rows"] = n_rows
        if peak_bar is not None:
            print(f"{label}: worst peak deviation from the pieces {res['worst_peak']:.2e} (bar {peak_bar[0]:.0e})")
        print(f"{label}: worst mix figure {res['worst_mix']:.3e} (TOL {TOL:.0e}), peaks bitwise those of the pieces: {res['peaks_bitwise']}, worst anchor deviation {res['worst_anchor']:.2e} of the oracle's (bar {anchor_bar[0]:.0e}), {n_rows} partial rows, kernel {prof['kernel']!r}")
        assert not outside, "\n".join(outside)
        return res
    finally:
        for ctx in ctxs:
            ctx.close()
