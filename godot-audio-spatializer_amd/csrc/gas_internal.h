// gas_internal.h -- context layout and kernel launchers shared by the csrc/ translation units.
// Not part of the ABI (include/gas_amd.h is).
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/gas_amd.h"

static_assert(sizeof(gas_params) == 128, "gas_params is a 128-byte POD");
static_assert(sizeof(gas_audio_frame) == 8, "AudioFrame is 2 x f32");
static_assert(sizeof(gas_hrtf_blend) == 32, "gas_hrtf_blend is 4 directions and 4 weights: two 16-byte loads");
static_assert(sizeof(gas_fx_dyn_settings) == 12 * 4 * GAS_MAX_EFFECTS, "gas_fx_dyn_settings is 12 arrays by chain position");
static_assert(sizeof(gas_fx_line_settings) == 21 * 4 * GAS_MAX_EFFECTS, "gas_fx_line_settings is 21 arrays by chain position");
static_assert(sizeof(gas_fx_eq_settings) == 336, "gas_fx_eq_settings is [GAS_MAX_EFFECTS][21] f32");
static_assert(sizeof(gas_fx_mod_settings) == 512, "gas_fx_mod_settings is 5 arrays by chain position, 6 by position and voice, 5 by position");
static_assert(sizeof(gas_fx_stereo_settings) == 128, "gas_fx_stereo_settings is 8 arrays by chain position");
static_assert(sizeof(gas_fx_filter_settings) == 128, "gas_fx_filter_settings is 5 arrays by chain position and 12 reserved words");
static_assert(sizeof(gas_fx_settings) == 4 * 4 * GAS_MAX_EFFECTS, "gas_fx_settings is 4 arrays by chain position");
static_assert(sizeof(gas_fx_settings) % 16 == 0 && sizeof(gas_fx_dyn_settings) % 16 == 0 && sizeof(gas_fx_line_settings) % 16 == 0 && sizeof(gas_fx_eq_settings) % 16 == 0 && sizeof(gas_fx_mod_settings) % 16 == 0 && sizeof(gas_fx_stereo_settings) % 16 == 0 && sizeof(gas_fx_filter_settings) % 16 == 0, "k_scatter_fx moves a family's settings POD as 16-byte pieces");

// GAS_FX_EQ6 / _EQ10 / _EQ21 (k_fx_eq.hip): one bank of state per instance, [21 bands][a2, a3, b2, b3]
// [2 ears] floats (the engine's BandProcess history per band and ear), and the per-band coefficients of one preset at
// the context's mix rate (computed in f64, rounded to f32; 0 for a band whose formula has no real root)
#define GAS_EQ_BANK_FLOATS (GAS_EQ_MAX_BANDS * 8)
struct gas_eq_coefs {
	float c1[GAS_EQ_MAX_BANDS], c2[GAS_EQ_MAX_BANDS], c3[GAS_EQ_MAX_BANDS];
};

// GAS_FX_FILTER (k_fx_filter.hip): one bank of state per instance, [4 stages][a1, a2, b1, b2][2 ears]
// floats (the history of the engine's four AudioFilterSW processors per ear)
#define GAS_FILTER_BANK_FLOATS 32

// GAS_FX_CHORUS / GAS_FX_PHASER (k_fx_mod.hip).  A chorus line is GAS_CHORUS_HEADER floats of state
// {pos u32, -, cycles[4] u64, -, h[4 voices][2 ears] at GAS_CHORUS_H}, then a ring of chorus_mask + 1 stereo frames; a
// phaser bank is GAS_PHASER_BANK_FLOATS floats {phase, -, h[2 ears], zm1[6 stages][2 ears]}.
#define GAS_CHORUS_HEADER 64
#define GAS_CHORUS_H 16
#define GAS_PHASER_BANK_FLOATS 16

// GAS_FX_STEREO_ENHANCE (k_fx_stereo.hip).  A ring is GAS_ENHANCE_HEADER floats of state {pos u32, -,
// -, -}, then enhance_mask + 1 mono frames.
#define GAS_ENHANCE_HEADER 4

// k_zero_entries (k_misc.hip) writes a pool entry as float4: the entry sizes fixed at compile time are multiples of 4
// floats (the rings behind the two headers are powers of two, the line sizes multiples of 64: fx_reserve checks those)
static_assert(GAS_EQ_BANK_FLOATS % 4 == 0 && GAS_FILTER_BANK_FLOATS % 4 == 0 && GAS_CHORUS_HEADER % 4 == 0 && GAS_PHASER_BANK_FLOATS % 4 == 0 && GAS_ENHANCE_HEADER % 4 == 0, "pool entries are zeroed as float4");

// GAS_FX_DELAY / GAS_FX_REVERB line geometry, fixed per context by the mix rate (gas_ctx_reserve_fx_lines).
// Every line starts with GAS_LINE_HEADER floats of state; offsets below are in floats from the line's start.
#define GAS_LINE_HEADER 64
struct gas_line_geo {
	// delay line: header {P, q, h[2]}, ring [ring_mask + 1][2 ears], feedback buffer [fb_frames][2 ears]
	uint32_t ring_mask, fb_frames;
	size_t delay_floats;
	// reverb line: header {per ear e at 32 e: epos, h1, h2, comb pos[8], comb dh[8], allpass pos[4]}, then per ear
	// the echo buffer, the 8 combs and the 4 allpasses
	uint32_t echo_size;
	uint32_t xs[2]; // extra spread frames per ear
	uint32_t comb_size[2][8], ap_size[2][4];
	uint32_t echo_off[2], comb_off[2][8], ap_off[2][4];
	uint32_t ap_base[4]; // lrint(at[k] sr): the shortest limit allpass k can have
	size_t reverb_floats;
};

// ---------------------------------------------------------------------------
// Device-resident SpatializerPlaybackData (audio_spatializer_3d.h:85-99,
// audio_spatializer_effect.h:68-76), struct-of-arrays by "stream":
//   stream = (slot * 4 + channel_pair) * 2 + ear      (audio_spatializer_3d.cpp:887-894)
// so a wave of consecutive slots reads every field coalesced.
// ---------------------------------------------------------------------------
enum { GAS_BQ_FIELDS = 10 }; // b0 b1 b2 a1 a2 ha1 ha2 hb1 hb2 prev_vol
enum { BQ_B0 = 0, BQ_B1, BQ_B2, BQ_A1, BQ_A2, BQ_HA1, BQ_HA2, BQ_HB1, BQ_HB2, BQ_PREV };

// GAS_FLAG_ER_TAP_FADE: er_gain[8] as bits, then min(er_delay[8], er_ring_frames - frames); rendered != 0 once the words hold
// a row the stage rendered with.
struct gas_er_prev {
	uint32_t word[2 * GAS_ER_TAPS];
	uint32_t rendered;
};

struct gas_dev_state {
	float *bq; // [GAS_BQ_FIELDS][max_sources * 8]
	size_t bq_stride; // max_sources * 8
	float *hrtf_hist; // [max_sources][hist_len]   gained mono history
	float *hrtf_prev_gain; // [max_sources]
	uint32_t *hrtf_prev_dir; // [max_sources] previous callback's direction + 1 (0 = none), GAS_FLAG_HRTF_CROSSFADE
	gas_audio_frame *er_ring; // [max_sources][er_ring_frames]
	uint32_t *er_pos; // [max_sources]
	gas_params *params; // [max_sources]
	gas_fx_settings *fxs; // [max_sources] settings of the engine-effect kinds (GAS_FX_LOWPASS .. GAS_FX_AMPLIFY), by chain position
	uint8_t *was_further; // [max_sources] was_further_than_max_distance_last_frame (audio_spatializer_3d.h:118)
	// GAS_FX_DISTORTION / GAS_FX_COMPRESSOR (k_fx_dyn.hip): settings and the state that reaches the output
	gas_fx_dyn_settings *dyn; // [max_sources], by chain position
	float *dist_h; // [GAS_MAX_EFFECTS][2 ears][max_sources] the distortion's one-pole state h
	float *comp_rundb; // [GAS_MAX_EFFECTS][max_sources] the compressor's smoothed over-threshold level
	uint32_t dyn_stride; // max_sources
	gas_audio_frame *sidechain; // [GAS_MAX_SIDECHAINS][frames] the compressor's key blocks (gas_sidechain_set)
	// GAS_FX_DELAY / GAS_FX_REVERB (k_fx_line.hip): settings, slot -> line table, the two line pools (nullptr until
	// gas_ctx_reserve_fx_lines)
	gas_fx_line_settings *line_settings; // [max_sources], by chain position
	int32_t *line_of; // [GAS_MAX_EFFECTS][max_sources] line of chain position j in its kind's pool
	float *delay_pool; // [delay lines][geo.delay_floats]
	float *reverb_pool; // [reverb lines][geo.reverb_floats]
	// GAS_FX_EQ6 / _EQ10 / _EQ21 (k_fx_eq.hip): settings, slot -> bank table, the bank pool (nullptr until
	// gas_ctx_reserve_fx_eq)
	gas_fx_eq_settings *eq_settings; // [max_sources], by chain position
	int32_t *eq_of; // [GAS_MAX_EFFECTS][max_sources] bank of chain position j
	float *eq_pool; // [banks][GAS_EQ_BANK_FLOATS]
	// GAS_FX_CHORUS / GAS_FX_PHASER (k_fx_mod.hip): settings, slot -> line / bank table, the two pools (nullptr until
	// gas_ctx_reserve_fx_mod)
	gas_fx_mod_settings *mod_settings; // [max_sources], by chain position
	int32_t *mod_of; // [GAS_MAX_EFFECTS][max_sources] chorus line or phaser bank of chain position j
	float *chorus_pool; // [chorus lines][GAS_CHORUS_HEADER + 2 (chorus_mask + 1)]
	float *phaser_pool; // [phaser banks][GAS_PHASER_BANK_FLOATS]
	uint32_t chorus_mask; // ring frames - 1
	// GAS_FX_PANNER / GAS_FX_STEREO_ENHANCE / GAS_FX_LIMITER (k_fx_stereo.hip): settings and the slot -> ring table (from
	// gas_ctx_create on), the ring pool (nullptr until gas_ctx_reserve_fx_stereo)
	gas_fx_stereo_settings *stereo_settings; // [max_sources], by chain position
	int32_t *stereo_of; // [GAS_MAX_EFFECTS][max_sources] ring of chain position j, -1: none
	float *enhance_pool; // [rings][GAS_ENHANCE_HEADER + enhance_mask + 1]
	uint32_t enhance_mask; // ring frames - 1
	// GAS_FX_FILTER (k_fx_filter.hip): settings, slot -> bank table, the bank pool (nullptr until
	// gas_ctx_reserve_fx_filter)
	gas_fx_filter_settings *flt_settings; // [max_sources], by chain position
	int32_t *flt_of; // [GAS_MAX_EFFECTS][max_sources] bank of chain position j
	float *flt_pool; // [banks][GAS_FILTER_BANK_FLOATS]
	// GAS_FLAG_HRTF_INTERPOLATE: the HRIR rows each slot's HRTF stage blends (nullptr without the flag); read by
	// k_hrtf_ols_blend / k_hrtf_rows_blend, written by uploads and k_calc_spatialization only
	gas_hrtf_blend *hrtf_blend; // [max_sources], all-zero row = hrtf_dir at weight 1
	// GAS_FLAG_HRTF_BLEND_FADE: the effective row (compacted, clamped, {hrtf_dir, 1} for the all-zero row) each slot's HRTF
	// stage last rendered with, all-zero = none yet (nullptr without the flag); read and replaced by
	// k_hrtf_ols_blend_fade / k_hrtf_rows_blend_fade, zeroed with the slot's other DSP state (k_zero_slot)
	gas_hrtf_blend *hrtf_prev_blend; // [max_sources]
	// GAS_FLAG_ER_TAP_FADE: the effective tap row each slot's early-reflection stage last rendered with, and whether it has
	// rendered at all (an all-zero row is a legal tap set); nullptr without the flag.  Read and replaced by k_er_only<FADE>;
	// `rendered` is cleared with the slot's other DSP state (k_zero_slot)
	gas_er_prev *er_prev; // [max_sources]
};

// Device-resident playback cursor: what SpatialPlaybackListNode + the engine's sampler hold.
struct gas_cursor {
	const void *pcm; // stream base in HBM
	uint64_t frames; // stream length
	uint64_t pos; // frames consumed so far (fresh-frame cursor; the DSP sees pos - 64)
	uint64_t start; // first frame of this playback: the lookahead in front of it is zero (audio_spatializer.cpp:61-63)
	uint32_t format_channels; // format << 8 | channels
	uint32_t has_frames; // audio_spatializer.h:63
	// resampled playbacks ([ENGINE] AudioStreamPlaybackResampled): the engine's mix_offset, 16.16 fixed point, in frames
	// of the stream; and where / how fast the previous callback ran, from which its last 64 outputs (this callback's
	// lookahead, audio_spatializer.cpp:369-373) are regenerated instead of being stored
	uint64_t fp_pos, fp_prev_pos;
	uint32_t prev_inc;
	uint32_t resampled; // 0 plain, 1 resampled and never mixed yet (zeroed lookahead, :61-63), 2 resampled
	// NEW gas_stream_set_loop: pos / fp_pos / start count on the unrolled timeline U[k] = S[m(k)] and never wrap
	uint64_t loop_begin;
	uint32_t loop_len; // L = loop_end - loop_begin < 2^31
	uint32_t loop_mode; // gas_loop_mode; 0 = the stream plays once
};

// gas_source_feed_rows: the feed table a stream callback's kernels read, one device buffer.  Its header holds one word
// per list entry in the callback's row order: GAS_FEED_NONE, or where the entry's fed window row lies and how it is
// stored -- (offset from the table's base in 16-byte units) << 2 | (float32 ? 2 : 0) | (stereo ? 1 : 0).  The rows follow
// the header, [frames] each, every one 16-byte aligned.
#define GAS_FEED_NONE 0xffffffffu
__host__ __device__ inline uint32_t gas_feed_word(size_t byte_offset, int format, uint32_t channels) {
	return (uint32_t)(byte_offset >> 4) << 2 | (format == GAS_PCM_F32 ? 2u : 0u) | (channels == 2 ? 1u : 0u);
}
__host__ __device__ inline size_t gas_feed_offset(uint32_t word) {
	return (size_t)(word >> 2) << 4;
}
__host__ __device__ inline uint32_t gas_feed_format_channels(uint32_t word) { // gas_cursor::format_channels of the row
	return ((word & 2u ? (uint32_t)GAS_PCM_F32 : (uint32_t)GAS_PCM_S16) << 8) | ((word & 1u) + 1u);
}
__host__ __device__ inline size_t gas_feed_row_bytes(uint32_t word, uint32_t F) {
	return (size_t)F * (word & 2u ? 4u : 2u) * ((word & 1u) + 1u);
}

// The index map m of gas_stream_set_loop (gas_amd.h), and its incremental form for the frames of one window.
__host__ __device__ inline uint64_t gas_loop_map(uint64_t k, uint64_t b, uint32_t L, uint32_t mode) {
	if (mode == GAS_LOOP_DISABLED || k < b) {
		return k;
	}
	const uint64_t P = mode == GAS_LOOP_PINGPONG ? 2 * (uint64_t)L : L;
	const uint64_t t = (k - b) % P;
	return b + (t < L ? t : P - 1 - t);
}

// t(i) = (base + i - loop_begin) mod P (floored) for the frames i = 0 .. F of a window that starts at unrolled index
// `base`: the one 64-bit remainder of a source's callback.  The first `skip` frames lie in front of the loop (m = k).
struct gas_loop_win {
	uint32_t P, L, t0, skip, step;
};

__host__ __device__ inline gas_loop_win gas_loop_window(int64_t base, uint64_t b, uint32_t L, uint32_t mode, uint32_t F) {
	gas_loop_win w;
	w.L = L;
	w.P = mode == GAS_LOOP_PINGPONG ? 2 * L : L; // <= 2^32 - 2
	const int64_t d = base - (int64_t)b;
	if (d >= 0) {
		w.t0 = (uint32_t)((uint64_t)d % w.P);
		w.skip = 0;
	} else {
		const uint64_t nd = (uint64_t)-d;
		const uint32_t r = (uint32_t)(nd % w.P);
		w.t0 = r ? w.P - r : 0;
		w.skip = nd < F ? (uint32_t)nd : F;
	}
	w.step = w.P > 64 ? 64 : 64 % w.P; // a lane's frames are 64 apart
	return w;
}

// (t + a) mod P for t, a < P; the sum may carry out of 32 bits (P up to 2^32 - 2), the difference never does
__host__ __device__ inline uint32_t gas_loop_add(uint32_t t, uint32_t a, uint32_t P) {
	const uint32_t s = t + a;
	return (s < t || s >= P) ? s - P : s;
}

// t(lane), lane < 64: one conditional subtract when the period is longer than a wave, else a 32-bit remainder
__host__ __device__ inline uint32_t gas_loop_first(const gas_loop_win &w, uint32_t lane) {
	return w.P > 64 ? gas_loop_add(w.t0, lane, w.P) : (w.t0 + lane) % w.P;
}

__host__ __device__ inline uint32_t gas_loop_fold(const gas_loop_win &w, uint32_t t) {
	return t < w.L ? t : w.P - 1 - t;
}

// GAS_PCM_IMA_ADPCM (gas_amd.h): IMA/DVI ADPCM, the public standard.  A stream's device allocation holds the 4-bit codes
// padded with zeros to whole chunks of GAS_ADPCM_CHUNK frames (16 bytes per chunk and channel, so every chunk starts on
// a 16-byte boundary), then one checkpoint per chunk and channel: the decoder state in front of the chunk's first frame.
// Any frame is then at most GAS_ADPCM_CHUNK steps away from a known state, which is what lets the sampler read at
// arbitrary indices (loops, ping-pong, resampler taps).  20 bytes per 32 samples: 5 bits per sample.
#define GAS_ADPCM_CHUNK 32
#define GAS_ADPCM_STEPS 89
struct alignas(4) gas_adpcm_ckpt {
	int16_t predictor;
	uint8_t step_index;
	uint8_t pad;
};
static_assert(sizeof(gas_adpcm_ckpt) == 4, "gas_adpcm_ckpt layout");

__host__ __device__ inline uint64_t gas_adpcm_chunks(uint64_t frames) {
	return (frames + GAS_ADPCM_CHUNK - 1) / GAS_ADPCM_CHUNK;
}
// byte offset of the checkpoint table [chunk][channel] behind the codes
__host__ __device__ inline uint64_t gas_adpcm_table_offset(uint64_t frames, uint32_t channels) {
	return gas_adpcm_chunks(frames) * (GAS_ADPCM_CHUNK / 2) * channels;
}
__host__ __device__ inline uint64_t gas_adpcm_device_bytes(uint64_t frames, uint32_t channels) {
	return gas_adpcm_table_offset(frames, channels) + gas_adpcm_chunks(frames) * channels * sizeof(gas_adpcm_ckpt);
}

// The standard step-size table, 7 ... 32767.
__host__ __device__ inline int32_t gas_adpcm_step_size(uint32_t step_index) {
	static constexpr uint16_t STEP[GAS_ADPCM_STEPS] = { 7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767 };
	return STEP[step_index];
}

// One decoder step, the only definition of the arithmetic: code n moves (predictor, step_index); the sample is the new
// predictor.  `step` is gas_adpcm_step_size(step_index), looked up by the caller (the kernel keeps the table in LDS).
__host__ __device__ inline void gas_adpcm_step(int32_t &predictor, int32_t &step_index, uint32_t n, int32_t step) {
	const int32_t m = (int32_t)(n & 7);
	int32_t si = step_index + (m < 4 ? -1 : 2 * (m - 3)); // INDEX = {-1, -1, -1, -1, 2, 4, 6, 8}
	si = si < 0 ? 0 : si;
	step_index = si > GAS_ADPCM_STEPS - 1 ? GAS_ADPCM_STEPS - 1 : si;
	int32_t diff = step >> 3;
	diff += (n & 1) ? step >> 2 : 0;
	diff += (n & 2) ? step >> 1 : 0;
	diff += (n & 4) ? step : 0;
	int32_t p = predictor + ((n & 8) ? -diff : diff);
	p = p < -32768 ? -32768 : p;
	predictor = p > 32767 ? 32767 : p;
}

// Stream indices [lo, hi] that contain m(k) for every unrolled index k in [k0, k1] (0 <= k0 <= k1) of a looped cursor:
// the indices themselves in front of the loop; inside it the run they map to while no seam falls into it, else the
// whole loop.
__host__ __device__ inline void gas_stream_loop_bounds(const gas_cursor &c, uint64_t k0, uint64_t k1, uint64_t &lo, uint64_t &hi) {
	const uint64_t b = c.loop_begin;
	if (k1 < b) {
		lo = k0;
		hi = k1;
		return;
	}
	const uint64_t L = c.loop_len, P = c.loop_mode == GAS_LOOP_PINGPONG ? 2 * L : L;
	const uint64_t in0 = k0 > b ? k0 : b;
	const uint64_t t0 = (in0 - b) % P, t1 = t0 + (k1 - in0); // t runs t0 .. t1 before it wraps
	uint64_t mlo = b, mhi = b + L - 1;
	if (t1 < L) { // forward run
		mlo = b + t0;
		mhi = b + t1;
	} else if (t0 >= L && t1 < P) { // backward run of a ping-pong loop
		mlo = b + (P - 1 - t1);
		mhi = b + (P - 1 - t0);
	}
	lo = k0 < b ? k0 : mlo;
	hi = mhi;
}

// Bounds of the stream indices gas_sample_row (gas_sample_row.h) can load for this cursor and callback, hi < frames;
// false: it loads none.  What k_sample_adpcm.hip and k_sample_qoa.hip decode ahead of a row.
__host__ __device__ inline bool gas_stream_span_bounds(const gas_cursor &c, uint32_t F, uint64_t inc, uint64_t &lo, uint64_t &hi) {
	if (!c.has_frames) {
		return false;
	}
	int64_t k0, k1;
	if (c.resampled) { // taps q - 3 .. q of the fresh outputs, and of the regenerated lookahead once there is one
		const uint64_t fresh = F - GAS_LOOKAHEAD_BUFFER_SIZE;
		k0 = (int64_t)(c.fp_pos >> 16) - 3;
		k1 = (int64_t)((c.fp_pos + fresh * inc) >> 16);
		if (c.resampled == 2) {
			const int64_t p0 = (int64_t)((c.fp_prev_pos + fresh * c.prev_inc) >> 16) - 3, p1 = (int64_t)((c.fp_prev_pos + (uint64_t)F * c.prev_inc) >> 16);
			k0 = p0 < k0 ? p0 : k0;
			k1 = p1 > k1 ? p1 : k1;
		}
	} else { // the window
		k0 = (int64_t)c.pos - GAS_LOOKAHEAD_BUFFER_SIZE;
		k1 = k0 + (int64_t)F - 1;
	}
	if (k0 < (int64_t)c.start) {
		k0 = (int64_t)c.start;
	}
	if (!c.loop_mode && k1 > (int64_t)c.frames - 1) {
		k1 = (int64_t)c.frames - 1;
	}
	if (k1 < k0) {
		return false;
	}
	if (c.loop_mode) {
		gas_stream_loop_bounds(c, (uint64_t)k0, (uint64_t)k1, lo, hi);
	} else {
		lo = (uint64_t)k0;
		hi = (uint64_t)k1;
	}
	return true;
}

// What a launch group (one kind/chain) needs.
struct gas_group_args {
	const gas_audio_frame *src; // [n_rows_total][F]
	const uint32_t *rows; // [n] row of src per group entry, or nullptr (= identity)
	const uint32_t *slots; // [n] slot per group entry, or nullptr: slot = slot_base + entry (contiguous range)
	uint32_t slot_base;
	uint32_t n;
	float *peaks; // [n_rows_total][2]
	const uint32_t *peak_rows = nullptr; // k_hrtf_uni: [n] row of `peaks` per group entry when it differs from the row of src (a staged chain's last stage reads dense rows but reports into the callback's rows); nullptr = the src row
	const uint32_t *order = nullptr; // [n] processing order (k_hrtf_ols: entries grouped by HRIR direction; k_hrtf_uni: XCD-affine, k_xcd_order), or nullptr = entry order
};

// GAS_FLAG_PIPELINED_MIX: the final sum of the PREVIOUS callback's partial mixes (exactly k_mix_reduce's job for one
// channel pair), carried out by otherwise idle waves of this callback's k_hrtf_ols launch.  partials == nullptr: none.
#define GAS_HRTF_JOB_WAVES 4 // waves of a k_hrtf_ols workgroup that can each sum one output column of the previous callback
struct gas_deferred_reduce {
	const float *partials = nullptr; // [p_count][elems]
	uint32_t p_count = 0;
	uint32_t elems = 0; // F * 2
	float *out = nullptr;
};

enum gas_biquad_mode {
	GAS_MODE_MIX_CHANNEL = 0, // audio_spatializer_3d.cpp:554-609
	GAS_MODE_PROCESS_FRAMES = 1, // audio_spatializer_3d.cpp:491-552
	GAS_MODE_FX_HIGHSHELF = 2, // [ENGINE] AudioEffectFilterInstance::process, 1 stage
	GAS_MODE_COPY = 3, // empty effect chain, audio_spatializer_effect.cpp:41-46
	GAS_MODE_FX_FILTER = 4, // [ENGINE] AudioEffectFilterInstance::process of the other AudioFilterSW modes, 1 stage; settings from gas_fx_settings
	GAS_MODE_FX_AMPLIFY = 5, // [ENGINE] AudioEffectAmplifyInstance::process
};

struct gas_hrtf_table {
	float4 *spec; // [dirs][4][64] = (HL.re, HL.im, HR.re, HR.im) of bin lane + 64 j < 256, pre-scaled by 1/512; Nyquist in DC.imag
	uint32_t dirs;
};

static_assert(sizeof(gas_bus_route) == 8 + 32 + 4 * GAS_MAX_MORE_SENDS + 32 * GAS_MAX_MORE_SENDS, "gas_bus_route layout");

__host__ __device__ inline gas_bus_route gas_bus_route_default() { // a slot that never got a route: dry bus 0, no send
	gas_bus_route r{};
	r.dry_bus = 0;
	r.send_bus = GAS_BUS_NONE;
	for (int k = 0; k < GAS_MAX_MORE_SENDS; k++) {
		r.more_bus[k] = GAS_BUS_NONE;
	}
	return r;
}

// What a source sends to bus b for channel pair c and ear: dry 1 + the sends that name b, in field order.
__host__ __device__ inline float gas_bus_weight(const gas_bus_route &r, uint32_t b, int c, int ear) {
	float w = (r.dry_bus == b ? 1.0f : 0.0f) + (r.send_bus == b ? r.send[c][ear] : 0.0f);
#pragma unroll
	for (int k = 0; k < GAS_MAX_MORE_SENDS; k++) {
		w += r.more_bus[k] == b ? r.more_send[k][c][ear] : 0.0f;
	}
	return w;
}

// Several output buses: per-slot routes and how many buses the launch writes.  n_buses <= 1 is the
// single mix of gas_process_block (routes unused).  Partial layout with buses: plane (b * channel_count + c).
struct gas_bus_args {
	const gas_bus_route *routes = nullptr; // [max_sources], slot-indexed
	uint32_t n_buses = 1;
};

// Launchers (each only enqueues on `stream`; geometry is validated by the caller).
// Returns the number of partial mixes (per channel) it writes into `partials`
// ([C][P][F*2] floats, row stride P_stride).
uint32_t gas_biquad_partials(uint32_t n); // P for n sources
struct gas_biquad_launch {
	hipStream_t stream = nullptr;
	int mode = GAS_MODE_COPY;
	gas_group_args g{};
	const gas_dev_state *st = nullptr;
	uint32_t frames = 0;
	uint32_t channel_begin = 0, channel_count = 1; // a staged chain's stage passes its chain position as channel_begin
	float mix_rate = 0.0f;
	float *partials = nullptr;
	uint32_t p_offset = 0, p_stride = 0;
	float *rows_out = nullptr; // non-null: per-source rows instead of the partial mix
	gas_bus_args buses;
	int fx_kind = 0; // GAS_MODE_FX_FILTER: which GAS_FX_* filter
	bool scan_ok = true, pipe_ok = true; // the context's GAS_SHELF_SCAN / GAS_BIQUAD_PIPE (gas_switches.h): may the launcher choose k_shelf_scan / k_biquad_pipe
};
hipError_t gas_launch_biquad_mix(const gas_biquad_launch &a);

// k_shelf_scan.hip: a rows-out filter stage of a staged chain as a parallel scan over the frames (one wave per source),
// for callbacks too small to hide the serial recurrence (chosen inside gas_launch_biquad_mix)
bool gas_shelf_scan_applies(bool scan_ok, int mode, uint32_t n, uint32_t frames);
hipError_t gas_launch_shelf_scan(const gas_biquad_launch &a);

// k_biquad_pipe.hip: the same arithmetic as an eight-wave software pipeline per 32 sources, for callbacks with fewer
// workgroups than CUs (chosen inside gas_launch_biquad_mix)
bool gas_biquad_uses_pipe(bool pipe_ok, int mode, uint32_t n, uint32_t channel_count, uint32_t frames, bool rows_out); // the launcher's choice
hipError_t gas_launch_biquad_pipe(const gas_biquad_launch &a);

struct gas_hrtf_launch_plan {
	uint32_t wgs_fd, wgs_pk; // workgroups = partial mixes written
};
void gas_hrtf_plan(uint32_t n_fd, uint32_t n_pk, gas_hrtf_launch_plan *plan);
uint32_t gas_hrtf_partials(uint32_t n); // workgroups of a single-path launch (k_er_only, k_hrtf_rows, k_rows_accumulate)
// A fused launch ("sample inside the HRTF launch") reads no float rows.  Its kernels find, in g.src, the feed table when an
// entry of the list is fed, else the cursor array itself (k_hrtf_uni.hip: lane_cursor / fed_cursor).  The two launchers
// below pack their typed fields through here, and nobody else does.
inline const gas_audio_frame *gas_fused_src(const gas_cursor *cursors, const uint8_t *feed) {
	return feed ? reinterpret_cast<const gas_audio_frame *>(feed) : reinterpret_cast<const gas_audio_frame *>(cursors);
}
// What is the same for every HRTF launch of a context
struct gas_hrtf_launch_common {
	hipStream_t stream = nullptr;
	const gas_dev_state *st = nullptr;
	const gas_hrtf_table *tab = nullptr;
	const float2 *twiddles = nullptr;
	uint32_t frames = 0;
	uint32_t hist_len = 0;
	const float *fade_env = nullptr;
};
struct gas_hrtf_ols_launch : gas_hrtf_launch_common {
	bool with_er = false;
	bool crossfade = false;
	bool runs = false; // sum runs of equal directions before the FFT
	gas_group_args g_fd{}, g_pk{};
	uint32_t er_ring_frames = 0;
	float *partials = nullptr;
	uint32_t p_offset = 0;
	gas_cursor *cursors = nullptr; // non-null: sample the bound streams in the kernel (g_fd.src / g_pk.src are then unused)
	const gas_params *fresh = nullptr; // non-null: unscattered parameter rows in row order
	gas_deferred_reduce job;
	bool blend = false; // GAS_FLAG_HRTF_INTERPOLATE: k_hrtf_ols_blend (no cross-fade, no runs, no carried sum)
	bool fade = false; // GAS_FLAG_HRTF_BLEND_FADE, with blend only: k_hrtf_ols_blend_fade
};
hipError_t gas_launch_hrtf_ols(const gas_hrtf_ols_launch &a);
// k_hrtf_uni.hip: all plain [HRTF] sources of a callback in one uniform launch; peak_bits (bit per group entry, or
// nullptr) / peak_all say which sources also get their exact output peak
uint32_t gas_hrtf_uni_partials(uint32_t n); // workgroups (= partial mixes) of a k_hrtf_uni launch

// k_hrtf_multi.hip: K consecutive callbacks of one unchanged plain-[HRTF] list in one launch (GAS_FLAG_PIPELINED_MIX)
#define GAS_HRTF_MULTI_MAX_BLOCKS 16
struct gas_hrtf_blocks {
	uint32_t k = 0; // blocks in this launch
	const gas_audio_frame *src[GAS_HRTF_MULTI_MAX_BLOCKS] = {}; // [n][F] rows of block b
	const gas_params *fresh[GAS_HRTF_MULTI_MAX_BLOCKS] = {}; // device-published parameter rows taking effect at block b, or nullptr
	float *peaks[GAS_HRTF_MULTI_MAX_BLOCKS] = {}; // [n][2] of block b
	uint32_t p_offset[GAS_HRTF_MULTI_MAX_BLOCKS] = {}; // first partial row of block b (workgroup w writes row p_offset[b] + w)
	gas_deferred_reduce job[GAS_HRTF_MULTI_MAX_BLOCKS]; // pending sums of EARLIER launches carried by block b's idle waves
	const gas_params *last_fresh = nullptr; // the last non-null fresh[]: written through to the slot table at the end
};
// several independent deterministic sums (k_mix_reduce's) in one launch
struct gas_reduce_jobs {
	uint32_t count = 0;
	const float *partials[GAS_HRTF_MULTI_MAX_BLOCKS] = {}; // [p_count][F * 2] each
	uint32_t p_count[GAS_HRTF_MULTI_MAX_BLOCKS] = {};
	float *out[GAS_HRTF_MULTI_MAX_BLOCKS] = {};
};
hipError_t gas_launch_mix_reduce_jobs(hipStream_t stream, const gas_reduce_jobs &jobs, uint32_t frames);
bool gas_hrtf_multi_hist_in_lds(uint32_t n, uint32_t frames); // whether a launch over n sources keeps the history rows in LDS between its blocks
hipError_t gas_launch_hrtf_multi(hipStream_t stream, const gas_group_args &g, const gas_hrtf_blocks &mb, const uint32_t *peak_bits, bool peak_all, const gas_dev_state &st, const gas_hrtf_table &tab, const float2 *twiddles, uint32_t frames, uint32_t hist_len, float *partials);
struct gas_hrtf_uni_launch : gas_hrtf_launch_common {
	gas_group_args g{};
	const uint32_t *peak_bits = nullptr;
	bool peak_all = false;
	float *partials = nullptr;
	uint32_t p_offset = 0;
	gas_cursor *cursors = nullptr; // non-null: sample the bound streams in the kernel (g.src is then unused)
	const uint8_t *feed = nullptr; // with cursors only: the feed table when an entry of the list is fed (GAS_FEED_NONE, above)
	const gas_params *fresh = nullptr; // non-null: unscattered parameter rows in row order
	gas_deferred_reduce job;
	const gas_bus_route *routes = nullptr; // non-null: the two-bus form
	uint32_t bus_rows = 0;
	uint32_t bus_base = 0; // the launch's pair of buses: bus_base, bus_base + 1
	bool commit = true; // false: leave history / previous gain / peaks to a later pass
	uint32_t er_ring_frames = 0; // non-zero: the chain [EARLY_REFLECTIONS, HRTF]
	uint32_t peak_from = 0xffffffffu; // entries from here on report their exact peak
	uint32_t peak_bit_base = 0; // entry e's bit in peak_bits is bit e + peak_bit_base
	uint32_t flt_kind = 0; // non-zero: the chain [this one-biquad kind, HRTF]
	uint32_t flt_pos = 0; // its chain position (processor state, effect settings)
	float mix_rate = 0.0f;
};
hipError_t gas_launch_hrtf_uni(const gas_hrtf_uni_launch &a);
hipError_t gas_launch_er_only(hipStream_t stream, const gas_group_args &g, const gas_dev_state &st, uint32_t frames, uint32_t er_ring_frames, float *partials, uint32_t p_offset, uint32_t p_stride, gas_audio_frame *rows_out = nullptr, bool fade = false /* GAS_FLAG_ER_TAP_FADE */);
// stages of a general effect chain (rows in -> rows out) and its final mix
hipError_t gas_launch_hrtf_rows(hipStream_t stream, bool crossfade, const gas_group_args &g, const gas_dev_state &st, const gas_hrtf_table &tab, const float2 *twiddles, uint32_t frames, gas_audio_frame *rows_out, bool blend = false /* GAS_FLAG_HRTF_INTERPOLATE */, bool fade = false /* GAS_FLAG_HRTF_BLEND_FADE, with blend only */);
hipError_t gas_launch_rows_accumulate(hipStream_t stream, const gas_group_args &g, uint32_t frames, float *partials, uint32_t p_offset);
hipError_t gas_launch_rows_accumulate_buses(hipStream_t stream, const gas_group_args &g, uint32_t frames, const gas_bus_route *routes, uint32_t n_buses, uint32_t bus_rows, float *partials, uint32_t p_offset); // bus b's partial rows: [b * bus_rows + p_offset + workgroup]

hipError_t gas_launch_hrtf_table(hipStream_t stream, const float *d_hrir, uint32_t dirs, uint32_t taps, const float2 *twiddles, float4 *spec);
// k_conv.hip: the bus convolvers (gas_conv_*, NEW).  A spectrum is the Hermitian half of a 1024-point real
// transform: 512 float2, bin k at [k], the real Nyquist bin parked in the (zero) imaginary part of DC.
#define GAS_CONV_BINS 512
#define GAS_CONV_MAX_CHUNKS 32
enum : uint32_t { GAS_CONV_MONO = 0, GAS_CONV_STEREO = 1, GAS_CONV_TRUE_STEREO = 2 }; // an IR of 1, 2 or 4 channels
__host__ __device__ inline uint32_t gas_conv_mode(uint32_t channels) {
	return channels == 4 ? GAS_CONV_TRUE_STEREO : channels == 2 ? GAS_CONV_STEREO : GAS_CONV_MONO;
}
struct gas_conv_entry { // one named instance of a gas_conv_process call
	const float2 *H; // its IR's spectra [channels][k_ir][GAS_CONV_BINS], scaled by 1/512
	uint32_t slot; // instance: ring [slot][ear][K][GAS_CONV_BINS], previous block [slot][ear][512]
	uint32_t pos; // ring position this block's spectrum goes to
	uint32_t k_ir; // partitions of the IR, 1 .. K
	uint32_t mode; // GAS_CONV_MONO: both ears use channel 0; _STEREO: ear e uses channel e; _TRUE_STEREO: 2 i + e, both inputs i
	float dry, wet;
	// A fade in progress (gas_conv_fade_to): the fields above are state A, these state B; all zero where settled.
	const float2 *HB; // B's spectra; null where B names A's IR (a level-only fade: one wet sum serves both states)
	uint32_t k_irB, modeB;
	float dryB, wetB;
	uint32_t fade_t0; // frames of the fade before this call's frame 0: b F
	float fade_inv; // 1 / (N F), so that frame i has s = (float)(fade_t0 + i) * fade_inv; 0: settled
};
static_assert(sizeof(gas_conv_entry) == 64, "the call travels by value as a kernel argument (DESIGN.md 3.5k quotes its size)");
struct gas_conv_call { // passed by value: a device-memory call only enqueues, so nothing it reads may live in reused staging
	gas_conv_entry e[GAS_MAX_CONVOLVERS];
	uint8_t fading[GAS_MAX_CONVOLVERS]; // indices of the entries with a fade in progress, in call order (gas_launch_conv)
};
struct gas_conv_pool {
	float2 *ring = nullptr;
	float *prev = nullptr;
	// partial sums of one call, [GAS_MAX_CONVOLVERS * 4][max_chunks][GAS_CONV_BINS]: row 2 i + ear is entry i's sum over its
	// IR (state A while it fades), row 2 GAS_MAX_CONVOLVERS + 2 i + ear its sum over state B's IR while it fades
	float2 *ypart = nullptr;
	const float2 *w1024 = nullptr; // [512] exp(-2 pi i k / 1024)
	uint32_t K = 0; // partitions per ring: ceil(max_ir_taps / frames)
	uint32_t max_chunks = 0; // gas_conv_max_chunks(K)
};
// The multiply-accumulate walks an IR's partitions in chunks, one workgroup row per chunk, and the inverse stage adds the
// chunks' sums in chunk order.  The split depends on the IR's length alone, so an instance's bits do not depend on what
// else a call names.
__host__ __device__ inline uint32_t gas_conv_chunk_len(uint32_t k_ir) {
	const uint32_t per = (k_ir + GAS_CONV_MAX_CHUNKS - 1) / GAS_CONV_MAX_CHUNKS;
	return per < 16 ? 16 : per;
}
__host__ __device__ inline uint32_t gas_conv_chunks(uint32_t k_ir) {
	const uint32_t len = gas_conv_chunk_len(k_ir);
	return (k_ir + len - 1) / len;
}
__host__ __device__ inline uint32_t gas_conv_max_chunks(uint32_t K) { // the most chunks any IR of at most K partitions has
	const uint32_t c = (K + 15) / 16;
	return c < GAS_CONV_MAX_CHUNKS ? c : GAS_CONV_MAX_CHUNKS;
}
// fills call.fading from the entries' fade_inv
hipError_t gas_launch_conv(hipStream_t stream, gas_conv_call &call, uint32_t n, const gas_conv_pool &pool, const float2 *twiddles, const gas_audio_frame *in /* [n][frames] */, gas_audio_frame *out /* [n][frames] */, uint32_t frames);
hipError_t gas_launch_conv_ir(hipStream_t stream, const float *d_ir /* [channels][taps] */, uint32_t channels, uint32_t taps, uint32_t frames, const float2 *twiddles, const float2 *w1024, float2 *H);
void gas_make_w1024(float2 *host_w /* [512] */);
hipError_t gas_launch_hrtf_regrid(hipStream_t stream, const float *d_positions, const float *d_hrir, uint32_t m, uint32_t taps, uint32_t az_steps, uint32_t el_steps, int interpolation, float *d_out /* [az_steps * el_steps][2][GAS_HRTF_TAPS] */);
void gas_make_twiddles(float2 *host_tw /* [64][16] */);

hipError_t gas_launch_mix_reduce(hipStream_t stream, const float *partials, uint32_t p_count, uint32_t p_stride, uint32_t channels, uint32_t frames, gas_audio_frame *out);
// k_fx_dyn.hip: a GAS_FX_DISTORTION / GAS_FX_COMPRESSOR stage of a staged chain (rows in -> dense rows out), settings
// and state of chain position chain_pos
hipError_t gas_launch_fx_dyn(hipStream_t stream, int kind, const gas_group_args &g, const gas_dev_state &st, uint32_t frames, uint32_t chain_pos, float mix_rate, gas_audio_frame *rows_out);
// The effect families share k_misc.hip's settings scatter and zeroing.  k_scatter_fx: [n] settings PODs
// of pod_bytes (a multiple of 16) go to settings_table[slot], [n] {slot, entry[GAS_MAX_EFFECTS]} rows to the
// [GAS_MAX_EFFECTS][stride] table of_table (nullptr: a family without pools, the entries are skipped).  k_zero_entries:
// [z] {pool, entry} records, entry_floats[pool] floats (a multiple of 4) of pools[pool] each; z == 0 launches nothing.
hipError_t gas_launch_scatter_fx(hipStream_t stream, void *settings_table, int32_t *of_table, uint32_t stride, uint32_t pod_bytes, const void *upload, const uint32_t *slot_idx, uint32_t n);
hipError_t gas_launch_zero_entries(hipStream_t stream, float *const pools[2], const size_t entry_floats[2], const uint32_t *records, uint32_t z);
// k_fx_line.hip: a GAS_FX_DELAY / GAS_FX_REVERB stage (rows in -> dense rows out)
hipError_t gas_launch_fx_line(hipStream_t stream, int kind, const gas_group_args &g, const gas_dev_state &st, const gas_line_geo &geo, uint32_t frames, uint32_t chain_pos, float mix_rate, gas_audio_frame *rows_out);
// k_fx_eq.hip: a GAS_FX_EQ6 / _EQ10 / _EQ21 stage (rows in -> dense rows out) with the preset's coefficients
hipError_t gas_launch_fx_eq(hipStream_t stream, int kind, const gas_group_args &g, const gas_dev_state &st, const gas_eq_coefs &coefs, uint32_t frames, uint32_t chain_pos, gas_audio_frame *rows_out);
int gas_eq_bands(int kind); // 6, 10, 21; 0 for any other kind
// k_fx_mod.hip: a GAS_FX_CHORUS / GAS_FX_PHASER stage (rows in -> dense rows out)
hipError_t gas_launch_fx_mod(hipStream_t stream, int kind, const gas_group_args &g, const gas_dev_state &st, uint32_t frames, uint32_t chain_pos, float mix_rate, gas_audio_frame *rows_out);
// k_fx_stereo.hip: a GAS_FX_PANNER / GAS_FX_STEREO_ENHANCE / GAS_FX_LIMITER stage (rows in -> dense rows out)
hipError_t gas_launch_fx_stereo(hipStream_t stream, int kind, const gas_group_args &g, const gas_dev_state &st, uint32_t frames, uint32_t chain_pos, float mix_rate, gas_audio_frame *rows_out);
// k_fx_filter.hip: a GAS_FX_FILTER stage (rows in -> dense rows out)
hipError_t gas_launch_fx_filter(hipStream_t stream, const gas_group_args &g, const gas_dev_state &st, uint32_t frames, uint32_t chain_pos, float mix_rate, gas_audio_frame *rows_out);
hipError_t gas_launch_scatter_params(hipStream_t stream, gas_params *table, const gas_params *upload, const uint32_t *slots, uint32_t n);
hipError_t gas_launch_calc_spatialization(hipStream_t stream, const gas_spatializer3d_config *cfgs, const uint32_t *cfg_index, const gas_source_pose *poses, const gas_listener *listeners, uint32_t n_listeners, const uint32_t *slots, uint32_t n, gas_params *table, uint8_t *was_further, gas_params *out_params, const gas_area_send *areas = nullptr, const float *listener_area_pos = nullptr, gas_audio_frame *out_reverb = nullptr, gas_hrtf_blend *blend_table = nullptr /* GAS_FLAG_HRTF_INTERPOLATE: the slots' bilinear blend rows are written too */);
// k_calc_er.hip: table == nullptr: nothing but out_taps is written (slots is not read); max_delay = er_ring_frames - frames
hipError_t gas_launch_calc_er(hipStream_t stream, const gas_room *rooms, const uint32_t *room_index, const gas_source_pose *poses, const gas_listener *listener, const uint32_t *slots, uint32_t n, uint32_t max_delay, float rate, gas_params *table, gas_er_taps *out_taps);
// k_room_ir.hip: gas_conv_ir_from_room.  The plan is steps 1 and 2 of the rule, made on the host in float64 and passed
// to the kernel by value.  gas_room_ir_make_plan is false for what the geometry refuses: a point outside the box,
// d0 < 1e-3, a candidate box of more than GAS_ROOM_IR_MAX_CELLS cells (the descriptor's plain fields are the caller's to
// check first).  The tables are gas_room_ir_table_doubles(plan) doubles: per axis, index m + N_a, the walls' reflectances
// an image with that m_a has met.  gas_launch_room_ir zeroes d_acc [channels][taps], accumulates, and writes d_out
// [channels][taps] f32, all in stream order.
#define GAS_ROOM_IR_MAX_CELLS (1u << 28)
struct gas_room_ir_plan {
	double h[3], s[3], e[2][3]; // half extents, source, receivers (both the listener for one channel), in the room's frame
	double d0, c, rate, level;
	uint32_t N[3], cells; // (2 N_x + 1)(2 N_y + 1)(2 N_z + 1) <= GAS_ROOM_IR_MAX_CELLS
	uint32_t min_order, max_order, channels, taps;
};
bool gas_room_ir_make_plan(const gas_room_ir &desc, uint32_t channels, uint32_t taps, float rate, gas_room_ir_plan &plan);
size_t gas_room_ir_table_doubles(const gas_room_ir_plan &plan);
void gas_room_ir_fill_tables(const gas_room_ir &desc, const gas_room_ir_plan &plan, double *host_tables);
hipError_t gas_launch_room_ir(hipStream_t stream, const gas_room_ir_plan &plan, const double *d_tables, long long *d_acc, float *d_out);
// step 6 alone, for every generator that leaves int64 sums of shares: d_out[i] = (float)(level d_acc[i] 2^-32), i < n
hipError_t gas_launch_room_ir_scale(hipStream_t stream, const long long *d_acc, uint32_t n, double level, float *d_out);
// k_room_planes.hip: gas_conv_ir_from_planes.  The plan is step 1 of the rule (normalised planes, source, receivers, d0)
// and the layout of the candidates, made on the host in float64 and passed to the kernel by value.  A candidate's flat
// index is first[K] + r, K its order and r its digits, most significant first: the first base P, the later ones base
// P - 1 and mapped past the plane before them.  gas_room_planes_make_plan is false for what the geometry refuses: a
// normal's length outside [0.999, 1.001], the source or a receiver not strictly inside every half-space, d0 < 1e-3, more
// than GAS_ROOM_PLANES_MAX_CANDIDATES sequences (the descriptor's plain fields are the caller's to check first).
// gas_launch_room_planes zeroes d_acc [channels][taps], accumulates, and writes d_out [channels][taps] f32, all in
// stream order.
#define GAS_ROOM_PLANES_MAX_CANDIDATES (1u << 28)
struct gas_room_planes_plan {
	double n[GAS_ROOM_MAX_PLANES][3], d[GAS_ROOM_MAX_PLANES], refl[GAS_ROOM_MAX_PLANES];
	double s[3], e[2][3]; // source, receivers (both the listener for one channel)
	double d0, c, rate, level;
	double far2; // (c (taps + 1) / rate + d0)^2: an image further than this from every receiver reaches no tap, nor does one made from it
	uint32_t first[GAS_ROOM_PLANES_MAX_ORDER + 2]; // [K], lo <= K <= hi + 1: first[lo] = 0, first[hi + 1] = candidates
	uint32_t pw[GAS_ROOM_PLANES_MAX_ORDER]; // (P - 1)^k
	uint32_t P, lo, hi, candidates; // orders lo .. hi, lo = max(min_order, 1)
	uint32_t direct; // min_order == 0: candidate 0's lane adds the direct sound as well
	uint32_t channels, taps;
};
bool gas_room_planes_make_plan(const gas_room_planes &desc, uint32_t channels, uint32_t taps, float rate, gas_room_planes_plan &plan);
hipError_t gas_launch_room_planes(hipStream_t stream, const gas_room_planes_plan &plan, long long *d_acc, float *d_out);
// gas_conv_ir_from_room_hrtf: the plan is made with channels = 1 (one receiver, the listener); d_acc and d_out are
// [2][taps] all the same, one row per ear.  d_hrir is the set as the caller passed it, f32 [n_az * n_el][2][hrir_taps];
// the two bases of `desc` travel to the kernel widened, by value.
struct gas_room_ir_frames {
	double B[3][3], L[3][3]; // room.basis, listener.basis
};
hipError_t gas_launch_room_ir_hrtf(hipStream_t stream, const gas_room_ir_plan &plan, const gas_room_ir &desc, const double *d_tables, const float *d_hrir, uint32_t n_az, uint32_t n_el, uint32_t hrir_taps, long long *d_acc, float *d_out);
// k_room_bands.hip: gas_conv_ir_from_room_bands and gas_conv_ir_from_room_hrtf_bands.  d_acc is [bands][channels][taps],
// band b's sums as gas_launch_room_ir[_hrtf] left them; d_filt is [bands][Lp] as gas_room_bands_fill_filters wrote it on
// the host (step 3: row b reversed and padded with zeros to Lp).  B == 1 has L = 1, D = 0 whatever filter_taps says.
// gas_launch_room_bands_combine writes d_out [channels][taps] f32 (steps 2, 4 and 5), in stream order.
#define GAS_ROOM_BANDS_TILE 1792u // output taps per workgroup of the combine kernel from GAS_ROOM_BANDS_WIDE_FROM outputs on
#define GAS_ROOM_BANDS_SMALL_TILE 256u // and below that
#define GAS_ROOM_BANDS_WIDE_FROM (1u << 19) // channels * taps
#define GAS_ROOM_BANDS_FILTER_STEP 16u
struct gas_room_bands_plan {
	double lambda[GAS_ROOM_MAX_BANDS]; // step 2's lambda_b
	double level;
	uint32_t bands, channels, taps;
	uint32_t L, D, Lp; // Lp = L rounded up to GAS_ROOM_BANDS_FILTER_STEP
};
void gas_room_bands_fill_filters(const gas_room_bands &bands, double rate, const gas_room_bands_plan &plan, double *host_filt);
hipError_t gas_launch_room_bands_combine(hipStream_t stream, const gas_room_bands_plan &plan, const long long *d_acc, const double *d_filt, float *d_out);
// k_room_tail.hip: gas_conv_ir_from_room_diffuse and gas_conv_ir_from_room_hrtf_diffuse.  gas_room_tail_marks is step 1's
// K0 and K1; false for what a gas_room_tail is refused for on its own: a field that is negative or not finite,
// reserved != 0 (a NULL tail is the caller's to refuse first).  gas_room_tail_make_plan is step 3 on the host in float64
// from the lattice plan's geometry (h, d0, c, rate; its taps are not read); false for s0 not finite or above
// GAS_ROOM_TAIL_S0_MAX.
// gas_launch_room_tail reads d_spec [bands][channels][K1], band b's sums as gas_launch_room_ir[_hrtf] left them for a plan
// of K1 taps (not read when K1 == 0), and writes every element of d_acc [bands][channels][taps] (steps 4 - 6), in stream
// order; gas_launch_room_bands_combine takes it from there.
#define GAS_ROOM_TAIL_S0_MAX 1024.0
struct gas_room_tail_plan {
	double mu[GAS_ROOM_MAX_BANDS]; // step 3's mu_b; not read for a band of `dead`
	double s0, d0, c, rate;
	uint32_t seed, K0, K1;
	uint32_t bands, channels, taps;
	uint32_t dead; // bit b: rho_b == 0, the band's diffuse part is 0
};
bool gas_room_tail_marks(const gas_room_tail &tail, double rate, uint32_t taps, uint32_t &K0, uint32_t &K1);
bool gas_room_tail_make_plan(const gas_room_ir_plan &geometry, const gas_room_bands &bands, const gas_room_tail &tail, uint32_t channels, uint32_t taps, uint32_t K0, uint32_t K1, gas_room_tail_plan &plan);
hipError_t gas_launch_room_tail(hipStream_t stream, const gas_room_tail_plan &plan, const long long *d_spec, long long *d_acc);
hipError_t gas_launch_sample_sources(hipStream_t stream, gas_cursor *cursors, const uint32_t *slots, uint32_t n, uint32_t frames, const float *fade_env, gas_audio_frame *rows, const uint32_t *row_inc /* 16.16 step per row for resampled playbacks, or nullptr */, const uint8_t *feed = nullptr /* the feed table when an entry of the list is fed (GAS_FEED_NONE, above) */);
hipError_t gas_launch_sample_adpcm(hipStream_t stream, gas_cursor *cursors, const uint32_t *slots, uint32_t n, uint32_t frames, const float *fade_env, gas_audio_frame *rows, const uint32_t *row_inc, bool span /* false: every load decodes from its checkpoint (GAS_ADPCM_SPAN=0) */); // the GAS_PCM_IMA_ADPCM rows of the same list, after gas_launch_sample_sources
hipError_t gas_launch_sample_qoa(hipStream_t stream, gas_cursor *cursors, const uint32_t *slots, uint32_t n, uint32_t frames, const float *fade_env, gas_audio_frame *rows, const uint32_t *row_inc, bool span /* false: every load decodes from its record (GAS_QOA_SPAN=0) */); // the GAS_PCM_QOA rows of the same list, after gas_launch_sample_sources
hipError_t gas_launch_noop(hipStream_t stream); // event-timer calibration
hipError_t gas_launch_stream_probe(hipStream_t stream, const void *rd, uint64_t rd_bytes, void *wr, uint64_t wr_bytes, uint32_t workgroups, uint32_t unroll, float *sink); // copy-bandwidth ceiling
#define GAS_DIR_ORDER_SEGMENT 8192
#define GAS_DIR_ORDER_MIN_SOURCES 512
bool gas_dir_order_supported(uint32_t dirs);
// k_xcd_order (k_misc.hip): XCD-affine processing order for a k_hrtf_uni launch of hrtf_wgs workgroups (multiple of 8)
hipError_t gas_launch_xcd_order(hipStream_t stream, const gas_group_args &g, const gas_params *params, const gas_params *fresh, uint32_t dirs, uint32_t hrtf_wgs, uint32_t waves_per_wg, uint32_t *order);
uint32_t gas_hrtf_uni_waves();
bool gas_hrtf_uni_twelve(uint32_t n, bool streams, bool buses); // whether a callback of n plain-[HRTF] sources runs k_hrtf_uni's twelve-wave form (its sums differ from the eight-wave form's in the last bits)
hipError_t gas_launch_dir_order(hipStream_t stream, const gas_group_args &g, const gas_params *params, const gas_params *fresh, uint32_t dirs, uint32_t *order);
hipError_t gas_launch_zero_slot(hipStream_t stream, const gas_dev_state &st, uint32_t slot, uint32_t hist_len, uint32_t er_ring_frames);
