// k_sample_qoa.hip -- k_sample_sources' rows for GAS_PCM_QOA streams (gas_amd.h): the same row logic (gas_sample_row.h),
// launched behind k_sample_sources (and k_sample_adpcm) over the same list; each kernel leaves at once on the others'
// rows.
//
// The QOA decoder is a serial recurrence -- a 4-tap sign-LMS predictor whose weights move with every sample -- and the
// sampler reads frames at arbitrary indices, so the stream is kept as one 64-byte record per GAS_QOA_CHUNK = 80 frames
// and channel: the chunk's 4 slices as stored and the decoder state in front of them (gas_qoa.h: the layout and the one
// decoder step, shared with the record builder in gas_stream_create).  Two ways to a frame, chosen per row on
// wave-uniform values:
//
// per-load  the definition, right for any index: read record idx / 80, run idx % 80 + 1 steps (gas_qoa_record_sample).
// span      the wave bounds the stream indices its row can load (gas_stream_span_bounds, gas_internal.h: any superset
//           will do); if they cover at most SPAN_CHUNKS = 32 chunks (2560 frames), one lane per chunk and channel
//           decodes its record once, all of its slices, into wave-private LDS, one 32-bit word (left, right as int16;
//           mono twice the same) per frame, and every load of the row reads LDS.  A slice's 20 dequantised residuals do
//           not depend on the decoder state: they are looked up ahead of the recurrence, which keeps the multiply-adds
//           and the clamp alone on the serial chain (16 vector instructions and one DS write per step).
//           Wider ranges -- the seam of a long loop, a pitch near the top of the doppler clamp -- take the per-load path
//           for that row and callback.  GAS_QOA_SPAN=0 (read at context creation) forces per-load everywhere.
//
// Capacity: a plain row at F = 512 touches 8 chunks and a resampled one at pitch 4 touches 23; 32 covers both and keeps
// a workgroup at 41 KB of LDS (three workgroups per CU); a lane per chunk beyond 32 would need 64 x 81 words per wave.
//
// LDS layout of a span: chunk k's frame f at word k * 81 + f.  The decode writes lane-per-chunk: mono lane l < 32 writes
// whole words of chunk l; stereo lane l writes the 16-bit half of channel l >> 5 in chunk l & 31, so each group of 32
// lanes of a DS write holds one channel.  Word 81 k + f lies in bank (17 k + f) mod 32 and 17 is odd: the 32 lanes of a
// group hit 32 banks (a stride of 80 would fold them onto two).  The row reads frame-per-lane: consecutive lanes read
// consecutive frames, conflict-free inside a chunk.  The dequantisation table (128 words) sits in LDS once per
// workgroup.  4 waves x 10368 B + 512 B per workgroup.
#include "gas_qoa.h"
#include "gas_sample_row.h"

namespace {

constexpr uint32_t SPAN_CHUNKS = 32; // tests/qoa_ref.py mirrors it
constexpr uint32_t SPAN_STRIDE = GAS_QOA_CHUNK + 1;
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

struct qoa_src { // gas_sample_row's frame source
	const gas_qoa_record *recs; // [chunk][channel]
	uint32_t ch;
	const uint32_t *span; // LDS: this wave's decoded span
	uint64_t span_first; // stream frame of span[0]
	bool use_span;

	__device__ __forceinline__ gas_audio_frame load(uint64_t idx) const {
		if (use_span) {
			const uint32_t x = (uint32_t)(idx - span_first);
			const uint32_t w = span[(x / GAS_QOA_CHUNK) * SPAN_STRIDE + x % GAS_QOA_CHUNK];
			return to_frame((int16_t)(w & 0xffffu), (int16_t)(w >> 16));
		}
		const uint64_t chunk = idx / GAS_QOA_CHUNK;
		const uint32_t last = (uint32_t)(idx % GAS_QOA_CHUNK);
		if (ch == 1) {
			const int32_t v = gas_qoa_record_sample(recs[chunk], last);
			return to_frame(v, v);
		}
		return to_frame(gas_qoa_record_sample(recs[chunk * 2], last), gas_qoa_record_sample(recs[chunk * 2 + 1], last));
	}
};

// One lane per chunk and channel (see the header) decodes record chunk0 + k into span[k * 81 ..]: every slice that
// holds a frame of the stream, all 20 steps of it (the words of a partial last slice past the stream's end are written
// and never read).  deq: gas_qoa_dequant in LDS.  MONO is the stream's channel count, wave-uniform, taken out of the
// recurrence.
template <bool MONO>
__device__ __forceinline__ void decode_span(uint32_t *span, const int32_t *deq, const qoa_src &s, uint64_t chunk0, uint32_t n_chunks, uint64_t frames, uint32_t lane) {
	const uint32_t k = lane & 31, c = lane >> 5;
	if (k >= n_chunks || c >= s.ch) {
		return;
	}
	const uint64_t chunk = chunk0 + k;
	const uint64_t left = frames - chunk * GAS_QOA_CHUNK;
	const uint32_t cnt = left < GAS_QOA_CHUNK ? (uint32_t)left : GAS_QOA_CHUNK;
	const uint4 *q = reinterpret_cast<const uint4 *>(s.recs + chunk * s.ch + c);
	const uint4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
	const uint32_t dw[8] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w };
	gas_qoa_lms st;
	st.h[0] = (int16_t)(q2.x & 0xffffu);
	st.h[1] = (int16_t)(q2.x >> 16);
	st.h[2] = (int16_t)(q2.y & 0xffffu);
	st.h[3] = (int16_t)(q2.y >> 16);
	st.w[0] = (int32_t)q2.z;
	st.w[1] = (int32_t)q2.w;
	st.w[2] = (int32_t)q3.x;
	st.w[3] = (int32_t)q3.y;
	uint32_t *out = span + k * SPAN_STRIDE;
	uint16_t *half = reinterpret_cast<uint16_t *>(out) + c;
#pragma unroll
	for (uint32_t j = 0; j < GAS_QOA_CHUNK_SLICES; j++) {
		if (j * GAS_QOA_SLICE >= cnt) {
			break;
		}
		const uint64_t slice = ((uint64_t)__builtin_bswap32(dw[2 * j]) << 32) | __builtin_bswap32(dw[2 * j + 1]); // stored big-endian
		const int32_t *row = deq + gas_qoa_slice_sf(slice) * 8;
		int32_t d[GAS_QOA_SLICE];
#pragma unroll
		for (uint32_t i = 0; i < GAS_QOA_SLICE; i++) {
			d[i] = row[gas_qoa_slice_code(slice, i)];
		}
#pragma unroll
		for (uint32_t i = 0; i < GAS_QOA_SLICE; i++) {
			const uint32_t v = (uint32_t)gas_qoa_step(st, d[i]) & 0xffffu;
			const uint32_t f = j * GAS_QOA_SLICE + i;
			if (MONO) {
				out[f] = v * 0x10001u;
			} else {
				half[2 * f] = (uint16_t)v;
			}
		}
	}
}

__global__ __launch_bounds__(256) void k_sample_qoa(gas_cursor *__restrict__ cursors, const uint32_t *__restrict__ slots, uint32_t n, uint32_t F, const float *__restrict__ fade_env, gas_audio_frame *__restrict__ rows, const uint32_t *__restrict__ row_inc, int span_on) {
	__shared__ int32_t deq[GAS_QOA_DEQ_ENTRIES];
	__shared__ uint32_t spans[4 * SPAN_WORDS];
	if (threadIdx.x < GAS_QOA_DEQ_ENTRIES) {
		deq[threadIdx.x] = gas_qoa_dequant(threadIdx.x);
	}
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t e = blockIdx.x * 4 + wave;
	if (e >= n) {
		return;
	}
	gas_cursor *cp = cursors + slots[e];
	const gas_cursor c = *cp;
	if ((c.format_channels >> 8) != GAS_PCM_QOA) {
		return; // k_sample_sources' or k_sample_adpcm's row (a fed entry's too: its slot is unbound, the cursor all zero)
	}
	const uint32_t ch = c.format_channels & 0xff;
	const uint64_t inc = (c.resampled && row_inc) ? row_inc[e] : 65536u;
	uint32_t *span = spans + wave * SPAN_WORDS;
	qoa_src src{ static_cast<const gas_qoa_record *>(c.pcm), ch, span, 0, false };
	uint64_t lo = 0, hi = 0;
	if (span_on && c.pcm) {
		const bool any = gas_stream_span_bounds(c, F, inc, lo, hi);
		const uint64_t chunk0 = lo / GAS_QOA_CHUNK;
		const uint64_t n_chunks = any ? hi / GAS_QOA_CHUNK - chunk0 + 1 : 0;
		if (__builtin_amdgcn_readfirstlane((int)(n_chunks <= SPAN_CHUNKS))) {
			if (ch == 1) {
				decode_span<true>(span, deq, src, chunk0, (uint32_t)n_chunks, c.frames, lane);
			} else {
				decode_span<false>(span, deq, src, chunk0, (uint32_t)n_chunks, c.frames, lane);
			}
			wave_lds_sync();
			src.span_first = chunk0 * GAS_QOA_CHUNK;
			src.use_span = true;
		}
	}
	gas_sample_row(cp, c, rows + (size_t)e * F, F, (int)lane, inc, fade_env, src);
}

} // namespace

hipError_t gas_launch_sample_qoa(hipStream_t stream, gas_cursor *cursors, const uint32_t *slots, uint32_t n, uint32_t frames, const float *fade_env, gas_audio_frame *rows, const uint32_t *row_inc, bool span) {
	if (n == 0) {
		return hipSuccess;
	}
	hipLaunchKernelGGL(k_sample_qoa, dim3((n + 3) / 4), dim3(256), 0, stream, cursors, slots, n, frames, fade_env, rows, row_inc, span ? 1 : 0);
	return hipGetLastError();
}
