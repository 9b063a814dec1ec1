// k_sample_adpcm.hip -- k_sample_sources' rows for GAS_PCM_IMA_ADPCM streams (gas_amd.h): the same row logic
// (gas_sample_row.h), launched behind k_sample_sources over the same list; each kernel leaves at once on the other's rows.
//
// An ADPCM decoder is a serial integer recurrence and the sampler reads frames at arbitrary indices, so the stream
// carries the decoder state in front of every GAS_ADPCM_CHUNK = 32 frames (gas_internal.h: the layout and the one
// decoder step, shared with the table builder in gas_stream_create).  Two ways to a frame, chosen per row on wave-uniform
// values:
//
// per-load  the definition, right for any index: read checkpoint idx / 32, decode idx % 32 + 1 codes.
// span      the wave bounds the stream indices its row can load (gas_stream_span_bounds, gas_internal.h: any superset
//           will do); if they cover at most 64 chunks (2048 frames), lane l decodes chunk lo / 32 + l once, all 32 steps,
//           into wave-private LDS, one 32-bit word (left, right as int16; mono twice the same) per frame, and every
//           load of the row reads LDS.
//           Wider ranges -- the seam of a long loop, a pitch near the top of the doppler clamp -- take the per-load path
//           for that row and callback.  GAS_ADPCM_SPAN=0 (read at context creation) forces per-load everywhere.
//
// LDS layout of a span: chunk k's frame f at word k * 33 + f.  The decode writes lane-per-chunk (lane l, step f: word
// 33 l + f, bank (l + f) mod 32: the 32 lanes of a ds_write_b32 group hit 32 banks; a stride of 32 would put them all
// on one).  The row reads frame-per-lane: consecutive lanes read consecutive frames, bank (k + f) mod 32, which is
// conflict-free inside a chunk and 2-way on a single bank where a group of 32 lanes straddles two chunks (the pad word
// shifts the second chunk by one).  The step-size table (89 words) sits in LDS once per workgroup.  4 waves x 8448 B +
// 356 B per workgroup.
#include "gas_sample_row.h"

namespace {

constexpr uint32_t SPAN_CHUNKS = 64; // one per lane
constexpr uint32_t SPAN_STRIDE = GAS_ADPCM_CHUNK + 1;
constexpr uint32_t SPAN_WORDS = SPAN_CHUNKS * SPAN_STRIDE;

// Orders this wave's LDS traffic for the compiler; the hardware executes one wave's DS instructions in order.
__device__ __forceinline__ void wave_lds_sync() {
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ gas_audio_frame to_frame(int32_t l, int32_t r) {
	return gas_audio_frame{ (float)l / 32768.0f, (float)r / 32768.0f }; // as GAS_PCM_S16
}

// Code of frame f (< 32) of a chunk held as dwords: mono 4 dwords, 8 frames each; stereo 8 dwords, 4 frames each with
// byte (f >> 1) * 2 + channel (gas_amd.h).
__device__ __forceinline__ uint32_t mono_shift(uint32_t f) {
	return (f & 7) * 4;
}
__device__ __forceinline__ uint32_t stereo_shift(uint32_t f) {
	return ((f >> 1) & 1) * 16 + (f & 1) * 4; // left; right is 8 bits up
}

struct adpcm_src { // gas_sample_row's frame source
	const uint8_t *codes;
	const gas_adpcm_ckpt *table; // [chunk][channel]
	uint32_t ch;
	const int32_t *steps; // LDS: gas_adpcm_step_size
	const uint32_t *span; // LDS: this wave's decoded span
	uint64_t span_first; // stream frame of span[0]
	bool use_span;

	__device__ __forceinline__ gas_audio_frame load(uint64_t idx) const {
		if (use_span) {
			const uint32_t x = (uint32_t)(idx - span_first);
			const uint32_t w = span[(x / GAS_ADPCM_CHUNK) * SPAN_STRIDE + x % GAS_ADPCM_CHUNK];
			return to_frame((int16_t)(w & 0xffffu), (int16_t)(w >> 16));
		}
		const uint64_t chunk = idx / GAS_ADPCM_CHUNK;
		const uint32_t last = (uint32_t)(idx % GAS_ADPCM_CHUNK);
		uint32_t d = 0;
		if (ch == 1) {
			const gas_adpcm_ckpt k = table[chunk];
			const uint32_t *w = reinterpret_cast<const uint32_t *>(codes) + chunk * 4;
			int32_t p = k.predictor, si = k.step_index;
			for (uint32_t f = 0; f <= last; f++) {
				if ((f & 7) == 0) {
					d = w[f >> 3];
				}
				gas_adpcm_step(p, si, (d >> mono_shift(f)) & 15u, steps[si]);
			}
			return to_frame(p, p);
		}
		const gas_adpcm_ckpt kl = table[chunk * 2], kr = table[chunk * 2 + 1];
		const uint32_t *w = reinterpret_cast<const uint32_t *>(codes) + chunk * 8;
		int32_t pl = kl.predictor, sl = kl.step_index, pr = kr.predictor, sr = kr.step_index;
		for (uint32_t f = 0; f <= last; f++) {
			if ((f & 3) == 0) {
				d = w[f >> 2];
			}
			gas_adpcm_step(pl, sl, (d >> stereo_shift(f)) & 15u, steps[sl]);
			gas_adpcm_step(pr, sr, (d >> (stereo_shift(f) + 8)) & 15u, steps[sr]);
		}
		return to_frame(pl, pr);
	}
};

// Lane l < n_chunks decodes chunk chunk0 + l into span[l * 33 ..]; frames past the stream's end are not written.
__device__ __forceinline__ void decode_span(uint32_t *span, const adpcm_src &s, uint64_t chunk0, uint32_t n_chunks, uint64_t frames, uint32_t lane) {
	if (lane >= n_chunks) {
		return;
	}
	const uint64_t chunk = chunk0 + lane;
	const uint64_t left = frames - chunk * GAS_ADPCM_CHUNK;
	const uint32_t cnt = left < GAS_ADPCM_CHUNK ? (uint32_t)left : GAS_ADPCM_CHUNK;
	uint32_t *out = span + lane * SPAN_STRIDE;
	if (s.ch == 1) {
		const uint4 q = reinterpret_cast<const uint4 *>(s.codes)[chunk];
		const uint32_t w[4] = { q.x, q.y, q.z, q.w };
		const gas_adpcm_ckpt k = s.table[chunk];
		int32_t p = k.predictor, si = k.step_index;
#pragma unroll
		for (uint32_t f = 0; f < GAS_ADPCM_CHUNK; f++) {
			gas_adpcm_step(p, si, (w[f >> 3] >> mono_shift(f)) & 15u, s.steps[si]);
			if (f < cnt) {
				out[f] = ((uint32_t)p & 0xffffu) * 0x10001u;
			}
		}
		return;
	}
	const uint4 q0 = reinterpret_cast<const uint4 *>(s.codes)[chunk * 2], q1 = reinterpret_cast<const uint4 *>(s.codes)[chunk * 2 + 1];
	const uint32_t w[8] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w };
	const gas_adpcm_ckpt kl = s.table[chunk * 2], kr = s.table[chunk * 2 + 1];
	int32_t pl = kl.predictor, sl = kl.step_index, pr = kr.predictor, sr = kr.step_index;
#pragma unroll
	for (uint32_t f = 0; f < GAS_ADPCM_CHUNK; f++) {
		gas_adpcm_step(pl, sl, (w[f >> 2] >> stereo_shift(f)) & 15u, s.steps[sl]);
		gas_adpcm_step(pr, sr, (w[f >> 2] >> (stereo_shift(f) + 8)) & 15u, s.steps[sr]);
		if (f < cnt) {
			out[f] = ((uint32_t)pl & 0xffffu) | ((uint32_t)pr << 16);
		}
	}
}

__global__ __launch_bounds__(256) void k_sample_adpcm(gas_cursor *__restrict__ cursors, const uint32_t *__restrict__ slots, uint32_t n, uint32_t F, const float *__restrict__ fade_env, gas_audio_frame *__restrict__ rows, const uint32_t *__restrict__ row_inc, int span_on) {
	__shared__ int32_t steps[GAS_ADPCM_STEPS];
	__shared__ uint32_t spans[4 * SPAN_WORDS];
	if (threadIdx.x < GAS_ADPCM_STEPS) {
		steps[threadIdx.x] = gas_adpcm_step_size(threadIdx.x);
	}
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t e = blockIdx.x * 4 + wave;
	if (e >= n) {
		return;
	}
	gas_cursor *cp = cursors + slots[e];
	const gas_cursor c = *cp;
	if ((c.format_channels >> 8) != GAS_PCM_IMA_ADPCM) {
		return; // k_sample_sources' row (a fed entry's too: its slot is unbound, the cursor all zero)
	}
	const uint32_t ch = c.format_channels & 0xff;
	const uint64_t inc = (c.resampled && row_inc) ? row_inc[e] : 65536u;
	const uint8_t *codes = static_cast<const uint8_t *>(c.pcm);
	uint32_t *span = spans + wave * SPAN_WORDS;
	adpcm_src src{ codes, reinterpret_cast<const gas_adpcm_ckpt *>(codes + gas_adpcm_table_offset(c.frames, ch)), ch, steps, span, 0, false };
	uint64_t lo = 0, hi = 0;
	if (span_on && c.pcm) {
		const bool any = gas_stream_span_bounds(c, F, inc, lo, hi);
		const uint64_t chunk0 = lo / GAS_ADPCM_CHUNK;
		const uint64_t n_chunks = any ? hi / GAS_ADPCM_CHUNK - chunk0 + 1 : 0;
		if (__builtin_amdgcn_readfirstlane((int)(n_chunks <= SPAN_CHUNKS))) {
			decode_span(span, src, chunk0, (uint32_t)n_chunks, c.frames, lane);
			wave_lds_sync();
			src.span_first = chunk0 * GAS_ADPCM_CHUNK;
			src.use_span = true;
		}
	}
	gas_sample_row(cp, c, rows + (size_t)e * F, F, (int)lane, inc, fade_env, src);
}

} // namespace

hipError_t gas_launch_sample_adpcm(hipStream_t stream, gas_cursor *cursors, const uint32_t *slots, uint32_t n, uint32_t frames, const float *fade_env, gas_audio_frame *rows, const uint32_t *row_inc, bool span) {
	if (n == 0) {
		return hipSuccess;
	}
	hipLaunchKernelGGL(k_sample_adpcm, dim3((n + 3) / 4), dim3(256), 0, stream, cursors, slots, n, frames, fade_env, rows, row_inc, span ? 1 : 0);
	return hipGetLastError();
}
