"""GAS_FX_DELAY / GAS_FX_REVERB lines zeroed by gas_source_reset: repeated resets of one slot, and resets of every slot
after the pools are fully allocated, all before the next block.  Each line is queued for zeroing at most once, so the
upload of the next block stays within its buffer; the output must equal the reference run from zero state."""
import numpy as np
import pytest

import fx_line_ref as ref
from helpers import TOL, rel_rms

pytestmark = pytest.mark.gpu

DELAY, REVERB = 13, 14


def _run(gas, chain, n, F, resets, blocks=3, seed=0):
    from godot_audio_spatializer_amd import synth

    K = gas.capi
    rng = np.random.default_rng(seed)
    with gas.SpatializerContext(max_sources=n, frames=F) as ctx:
        ctx.reserve_fx_lines(n * chain.count(DELAY), n * chain.count(REVERB))  # every line of both pools taken
        slots = ctx.source_alloc_many(n, K.KIND_EFFECT, chain)
        ctx.params_publish_batch(slots, synth.draw_params(rng, n, dirs=8, frames=F))
        s = ref.draw_settings(rng, n, K)
        s["delay_feedback_active"] = 1
        ctx.fx_line_settings_publish(slots, s)
        stages = [ref.make_stage(k, j, n) for j, k in enumerate(chain)]

        def block():
            src = rng.uniform(-1, 1, (n, F, 2)).astype(np.float32)
            mix, _ = ctx.process_block(src, slots)
            x = src
            for st in stages:
                x = st.block(x, s)
            assert rel_rms(mix[0], x.astype(np.float64).sum(axis=0)) <= TOL

        for _ in range(resets):  # before the first block: the allocation's zeroing is still queued too
            for slot in slots:
                ctx.source_reset(int(slot))
        for _ in range(blocks):
            block()
        for _ in range(resets):  # a history, then the resets again
            for slot in slots:
                ctx.source_reset(int(slot))
        for st in stages:
            for i in range(n):
                st.reset(i)
        for _ in range(blocks):
            block()


def test_one_slot_reset_many_times_before_a_block(gas):
    _run(gas, (DELAY,), 1, 128, resets=6)


@pytest.mark.parametrize("chain", [(DELAY, DELAY, REVERB, REVERB), (REVERB, DELAY)])
def test_every_slot_of_full_pools_reset_before_a_block(gas, chain):
    _run(gas, chain, 6, 256, resets=3, seed=len(chain))
