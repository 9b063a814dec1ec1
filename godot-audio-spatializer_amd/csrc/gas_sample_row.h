// gas_sample_row.h -- the row logic of the stream sampler, shared by k_sample_sources.hip (GAS_PCM_S16 / GAS_PCM_F32)
// k_sample_adpcm.hip (GAS_PCM_IMA_ADPCM) and k_sample_qoa.hip (GAS_PCM_QOA): plain, looped and resampled branches, the fade table, the cursor write-back
// by lane 0; one wave per row.  Only where a frame comes from differs: `src.load(idx)` returns stream frame idx.
// What the rows are: k_sample_sources.hip's header.  Everything from here on is compiled with fp contract off, so a row
// is comparable bit for bit (tests/stream_window_ref.py).
#pragma once
#include "gas_internal.h"

// [ENGINE] AudioStreamPlaybackResampled::mix, one output frame at 16.16 position `off` (oracle: stream_mix_resampled):
// frames outside [start, len) read as zero.
#pragma clang fp contract(off)
template <class Src>
__device__ __forceinline__ gas_audio_frame gas_cubic_frame(const gas_cursor &c, const Src &src, uint64_t off) {
	const int64_t q = (int64_t)(off >> 16);
	const float mu = (float)(uint32_t)(off & 0xFFFFu) / 65536.0f;
	gas_audio_frame y[4];
	if (c.loop_mode) { // taps U[q-3 .. q] of the unrolled stream: one 64-bit remainder per output frame, then steps of one
		const gas_loop_win w = gas_loop_window(q - 3, c.loop_begin, c.loop_len, c.loop_mode, 4);
		const uint32_t one = w.P > 1 ? 1u : 0u;
		uint32_t t = w.t0;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const int64_t j = q - 3 + k;
			const uint64_t idx = (uint32_t)k < w.skip ? (uint64_t)j : c.loop_begin + gas_loop_fold(w, t);
			y[k] = j >= (int64_t)c.start ? src.load(idx) : gas_audio_frame{ 0.0f, 0.0f };
			t = gas_loop_add(t, one, w.P);
		}
	} else {
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const int64_t j = q - 3 + k;
			y[k] = (j >= (int64_t)c.start && j < (int64_t)c.frames) ? src.load((uint64_t)j) : gas_audio_frame{ 0.0f, 0.0f };
		}
	}
	const float mu2 = mu * mu;
	const float h11 = mu2 * (mu - 1);
	const float z = mu2 - h11;
	const float h01 = z - h11;
	const float h10 = mu - z;
	gas_audio_frame o;
	o.left = y[1].left + (y[2].left - y[1].left) * h01 + ((y[2].left - y[0].left) * h10 + (y[3].left - y[1].left) * h11) * 0.5f;
	o.right = y[1].right + (y[2].right - y[1].right) * h01 + ((y[2].right - y[0].right) * h10 + (y[3].right - y[1].right) * h11) * 0.5f;
	return o;
}

// Row `row` of the playback whose cursor is *cp (c: the copy the wave read); inc: this callback's 16.16 step (resampled
// playbacks only).
template <class Src>
__device__ __forceinline__ void gas_sample_row(gas_cursor *cp, const gas_cursor &c, gas_audio_frame *row, uint32_t F, int lane, uint64_t inc, const float *__restrict__ fade_env, const Src &src) {
	if (c.resampled && c.has_frames && c.pcm) {
		// The window the DSP sees is lookahead[64] ++ fresh[F] cut to F frames (audio_spatializer.cpp:367-378).  The fresh
		// frames are this call's outputs at positions fp_pos + i * inc; the lookahead is the previous call's last 64
		// outputs, regenerated from where and how fast that call ran.  The call reports as mixed the outputs produced
		// before the position's integer part first reaches the end of the stream.
		const uint64_t end_fp = c.frames << 16;
		uint64_t mixed64 = F;
		if (c.loop_mode) {
			// a looped playback never runs out
		} else if (c.fp_pos >= end_fp) {
			mixed64 = 0;
		} else if (inc > 0) {
			const uint64_t need = (end_fp - c.fp_pos + inc - 1) / inc; // first i with fp_pos + i * inc >= end
			mixed64 = need < F ? need : F;
		}
		const uint32_t mixed = (uint32_t)mixed64;
		for (uint32_t i = lane; i < F; i += 64) {
			gas_audio_frame v{ 0.0f, 0.0f };
			if (mixed == F || i < mixed + GAS_LOOKAHEAD_BUFFER_SIZE) { // valid frames end at 64 + mixed
				if (i >= GAS_LOOKAHEAD_BUFFER_SIZE) {
					v = gas_cubic_frame(c, src, c.fp_pos + (uint64_t)(i - GAS_LOOKAHEAD_BUFFER_SIZE) * inc);
				} else if (c.resampled == 2) {
					v = gas_cubic_frame(c, src, c.fp_prev_pos + (uint64_t)(F - GAS_LOOKAHEAD_BUFFER_SIZE + i) * c.prev_inc);
				}
				if (mixed != F && i >= mixed) { // :389-392
					const float f = fade_env[i - mixed];
					v.left *= f;
					v.right *= f;
				}
			}
			row[i] = v;
		}
		if (lane == 0) {
			cp->fp_prev_pos = c.fp_pos;
			cp->prev_inc = (uint32_t)inc;
			cp->fp_pos = c.fp_pos + (uint64_t)F * inc; // the engine advances over all requested frames
			cp->resampled = 2;
			if (mixed != F) {
				cp->has_frames = 0; // :398
			}
		}
		return;
	}
	if (c.loop_mode && c.has_frames && c.pcm) {
		// NEW gas_stream_set_loop: the same 64-frame delay over the unrolled stream, row[i] = S[m(pos - 64 + i)]; seams
		// fall wherever they fall and nothing fades or ends.  One 64-bit remainder per row, 32-bit steps per frame.
		const int64_t base = (int64_t)c.pos - GAS_LOOKAHEAD_BUFFER_SIZE;
		const gas_loop_win w = gas_loop_window(base, c.loop_begin, c.loop_len, c.loop_mode, F);
		uint32_t t = gas_loop_first(w, (uint32_t)lane);
		for (uint32_t i = lane; i < F; i += 64) {
			gas_audio_frame v{ 0.0f, 0.0f };
			const int64_t si = base + (int64_t)i;
			if (si >= (int64_t)c.start) {
				v = src.load(i < w.skip ? (uint64_t)si : c.loop_begin + gas_loop_fold(w, t));
			}
			row[i] = v;
			t = gas_loop_add(t, w.step, w.P);
		}
		if (lane == 0) {
			cp->pos = c.pos + F;
		}
		return;
	}
	uint32_t mixed = 0;
	if (c.has_frames && c.pcm) {
		const uint64_t left = c.frames > c.pos ? c.frames - c.pos : 0;
		mixed = left < F ? (uint32_t)left : F; // [ENGINE] AudioStreamPlayback::mix return value
	}
	for (uint32_t i = lane; i < F; i += 64) {
		gas_audio_frame v{ 0.0f, 0.0f };
		if (c.has_frames && c.pcm) {
			const int64_t si = (int64_t)c.pos - GAS_LOOKAHEAD_BUFFER_SIZE + (int64_t)i;
			if (mixed == F) {
				if (si >= (int64_t)c.start) {
					v = src.load((uint64_t)si);
				}
			} else if (i < mixed + GAS_LOOKAHEAD_BUFFER_SIZE) { // valid frames end at 64 + mixed
				if (si >= (int64_t)c.start) {
					v = src.load((uint64_t)si);
				}
				if (i >= mixed) { // :389-392
					const float f = fade_env[i - mixed];
					v.left *= f;
					v.right *= f;
				}
			} // else: buf[idx] *= 0.0 (:394) over the zero-filled tail
		}
		row[i] = v;
	}
	if (lane == 0 && c.has_frames) {
		cp->pos = c.pos + mixed;
		if (mixed != F) {
			cp->has_frames = 0; // :398
		}
	}
}
