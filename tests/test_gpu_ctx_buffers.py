"""One context whose buffers are allocated, grown, dropped and re-allocated while it runs (csrc/gas_owned.h behind
gas_ctx.hip and gas_ctx_*.hip), at the smallest shapes that cross the sites twice, all through host-memory calls:

  - an effect family reserved, released with a count of 0 and reserved larger, one callback of an [EQ6] chain against
    fx_eq_ref after each reservation (pool, settings, slot -> entry table and staging buffer dropped and re-made);
  - callbacks of 2, 16 and 2 playbacks of the chains [HRTF] and the staged [HIGHSHELF, ER] (the source staging, the
    partial mixes and the staged chains' ping-pong rows grow between the first two) against per-playback oracles;
  - the HRIR table swapped for a larger one between two callbacks: the later one matches oracles built from the new
    table (the [HRTF] playbacks are reset at the swap, so that new oracles start where they do);
  - window rows fed for one and then for four of the [HRTF] playbacks (gas_source_feed_rows: the pinned staging of a
    host-memory call grows), each followed by a stream callback over exactly the fed playbacks, which is
    gas_process_block on the same rows.

The context is then closed and the script replayed on a fresh one: every output equals the first pass bit for bit.

Sites that other tests already cross twice within one context are left to them: the bus partials
(test_gpu_buses.test_bus_call_reuses_the_list: two, then three buses), the probe arenas
(test_gpu_buses.test_probe_between_bus_callbacks_leaves_the_bus_buffers_alone), a stream destroyed and another created
in its place (test_gpu_stream_loops.test_rows_bitwise).  No failure of a runtime allocation is provoked here: those
paths are checked against a fake runtime in test_owned_host_program.py."""
import numpy as np
import pytest

import fx_eq_ref
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

HS, ER, HRTF, EQ6 = 1, 2, 3, 16
N, F, RING = 16, 128, 256
CHAINS = [((HRTF,), 8), ((HS, ER), 8)]


def _script(gas):
    """The session's inputs, drawn once and shared by both passes."""
    from godot_audio_spatializer_amd import synth

    rng = np.random.default_rng(58)
    K = gas.capi
    d = {"hrir": [synth.synthetic_hrir(np.random.default_rng(7 + dirs), dirs=dirs) for dirs in (8, 24)]}
    d["eq"] = [(fx_eq_ref.draw_settings(rng, n, K), synth.draw_params(rng, n, dirs=8, frames=F), rng.uniform(-1, 1, (n, F, 2)).astype(np.float32)) for n in (1, 3)]
    both = np.array([0, 8])  # one playback of each chain
    d["blocks"] = [(active, synth.draw_params(rng, N, dirs=dirs, ring_frames=RING, frames=F), synth.draw_sources(rng, N, F)) for active, dirs in ((both, 8), (np.arange(N), 8), (both, 8), (np.arange(N), 24), (both, 24))]
    d["feeds"] = [(np.arange(m), synth.draw_sources(rng, m, F)) for m in (1, 4)]
    return d


def _session(gas, ob, d, check):
    K = gas.capi
    assert (K.FX_HIGHSHELF, K.FX_EARLY_REFLECTIONS, K.FX_HRTF, K.FX_EQ6) == (HS, ER, HRTF, EQ6)
    outs = []
    empty = (np.zeros((0, F, 2), np.float32), np.zeros(0, np.uint32))
    with gas.SpatializerContext(max_sources=N, frames=F, er_ring_frames=RING) as ctx:
        for banks, (settings, p, src) in zip((1, 3), d["eq"]):
            ctx.reserve_fx_eq(banks)
            slots = ctx.source_alloc_many(banks, K.KIND_EFFECT, (EQ6,))
            ctx.params_publish_batch(slots, p)
            ctx.fx_eq_settings_publish(slots, settings)
            mix, _ = ctx.process_block(src, slots)
            if check:
                rows = fx_eq_ref.EqStage(EQ6, 0, banks, 48000.0).block(src, settings)
                assert rel_rms(mix[0], rows.astype(np.float64).sum(axis=0)) <= TOL, f"[EQ6], {banks} banks"
            outs.append(mix.copy())
            for s in slots:
                ctx.source_free(s)
            ctx.process_block(*empty)  # a block boundary: the slots and their banks are back
            ctx.reserve_fx_eq(0)

        ctx.hrtf_load(d["hrir"][0])
        slots = np.concatenate([ctx.source_alloc_many(m, K.KIND_EFFECT, ch) for ch, m in CHAINS])
        chain_of = [ch for ch, m in CHAINS for _ in range(m)]

        def oracles(hrir):
            return [ob.BatchOracle(ob.KIND_EFFECT, 1, F, chain=ch, hrir=hrir if HRTF in ch else None, er_ring_frames=RING) for ch in chain_of]

        oras = oracles(d["hrir"][0]) if check else None
        for t, (active, p, src) in enumerate(d["blocks"]):
            if t == 3:  # the larger table; the [ER] rings and shelves carry on, the HRTF histories start over
                ctx.hrtf_load(d["hrir"][1])
                for i in range(N):
                    if HRTF in chain_of[i]:
                        ctx.source_reset(slots[i])
                if check:
                    fresh = oracles(d["hrir"][1])
                    oras = [fresh[i] if HRTF in chain_of[i] else oras[i] for i in range(N)]
            ctx.params_publish_batch(slots, p)
            mix, _ = ctx.process_block(src[active], slots[active])
            if check:
                ref = np.zeros((F, 2))
                for i in active:
                    ref += oras[i].block(p[i : i + 1].astype(ob.PARAMS_DTYPE), src[i : i + 1], want64=True)[2][0]
                assert rel_rms(mix[0], ref) <= TOL, f"callback {t}"
            outs.append(mix.copy())
        p = d["blocks"][-1][1]
        for who, rows in d["feeds"]:
            ctx.source_feed_rows(slots[who], rows)
            mix, _, has_frames = ctx.process_block_streams(slots[who])
            assert has_frames.all()
            if check:
                ref = np.zeros((F, 2))
                for k, i in enumerate(who):
                    ref += oras[i].block(p[i : i + 1].astype(ob.PARAMS_DTYPE), rows[k : k + 1], want64=True)[2][0]
                assert rel_rms(mix[0], ref) <= TOL, f"{len(who)} fed rows"
            outs.append(mix.copy())
    return outs


def test_buffers_grow_and_are_replaced_inside_one_context(gas, ob):
    d = _script(gas)
    first = _session(gas, ob, d, check=True)
    again = _session(gas, ob, d, check=False)
    assert len(first) == len(again) == 9
    for t, (a, b) in enumerate(zip(first, again)):
        assert np.array_equal(a, b), f"output {t} of the second pass"
