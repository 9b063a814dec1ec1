// k_sample_sources.hip -- SURVEY.md 8f#2: the source window of _mix_from_playback_list
// (audio_spatializer.cpp:367-408) produced on the device from HBM-resident PCM streams.
//
// The reference keeps a 64-frame lookahead per playback so it can fade out when a stream ends abruptly:
//   buf = lookahead[64] ++ fresh[F];  the DSP consumes buf[0..F);  lookahead = buf[F..F+64)      (:369-378,:401-403)
// With the whole stream resident that is simply a 64-frame delay:  row[i] = S[pos - 64 + i]  (zero before the playback's
// start frame: the zeroed initial lookahead :61-63), where pos counts the fresh frames handed out so far.  When the stream runs
// out inside a callback (mixed = len - pos < F) the last 64 valid frames row[mixed .. mixed+64) are scaled by
// the reference's envelope 0.96^(j+1) * (64 - j) / 64 (:380-396; table computed on the host with the same f32
// recurrence), everything after is zero, and has_frames clears (:398); afterwards the row is all zeros (:405-408).
// One wave per playback row, lane-contiguous 8-byte stores; int16 -> float as s / 32768, mono feeds both ears.
// An entry with a row in the feed table (gas_source_feed_rows) takes that row instead, converted the same way: fed_row.
// The row logic itself is gas_sample_row.h's, shared with k_sample_adpcm.hip and k_sample_qoa.hip; this file reads the uncompressed formats.
#include "gas_sample_row.h"

namespace {

__device__ __forceinline__ gas_audio_frame load_frame(const void *pcm, uint32_t fmt, uint32_t ch, uint64_t idx) {
	if (fmt == GAS_PCM_S16) {
		const int16_t *p = static_cast<const int16_t *>(pcm);
		if (ch == 1) {
			const float v = (float)p[idx] / 32768.0f;
			return gas_audio_frame{ v, v };
		}
		const short2 s = reinterpret_cast<const short2 *>(p)[idx];
		return gas_audio_frame{ (float)s.x / 32768.0f, (float)s.y / 32768.0f };
	}
	const float *p = static_cast<const float *>(pcm);
	if (ch == 1) {
		const float v = p[idx];
		return gas_audio_frame{ v, v };
	}
	const float2 s = reinterpret_cast<const float2 *>(p)[idx];
	return gas_audio_frame{ s.x, s.y };
}

struct pcm_src { // gas_sample_row's frame source
	const void *pcm;
	uint32_t fmt, ch;
	__device__ __forceinline__ gas_audio_frame load(uint64_t idx) const {
		return load_frame(pcm, fmt, ch, idx);
	}
};

// gas_source_feed_rows: the window row of an entry that is not bound to a stream, converted from the feed table (the
// streams' conversion; no cursor is read or written).  A lane takes two frames per trip -- F is a multiple of 128 -- so
// every store is 16 bytes, and so is the load of a float32 stereo row.
__device__ __forceinline__ void fed_row(const uint8_t *__restrict__ feed, uint32_t word, gas_audio_frame *__restrict__ row, uint32_t F, int lane) {
	const uint8_t *p = feed + gas_feed_offset(word);
	for (uint32_t i = 2 * (uint32_t)lane; i < F; i += 128) {
		float4 v;
		switch (word & 3u) {
			case 0: { // int16 mono
				const short2 s = *reinterpret_cast<const short2 *>(p + (size_t)i * 2);
				const float a = (float)s.x / 32768.0f, b = (float)s.y / 32768.0f;
				v = make_float4(a, a, b, b);
			} break;
			case 1: { // int16 stereo
				const short4 s = *reinterpret_cast<const short4 *>(p + (size_t)i * 4);
				v = make_float4((float)s.x / 32768.0f, (float)s.y / 32768.0f, (float)s.z / 32768.0f, (float)s.w / 32768.0f);
			} break;
			case 2: { // float32 mono
				const float2 s = *reinterpret_cast<const float2 *>(p + (size_t)i * 4);
				v = make_float4(s.x, s.x, s.y, s.y);
			} break;
			default: // float32 stereo
				v = *reinterpret_cast<const float4 *>(p + (size_t)i * 8);
				break;
		}
		*reinterpret_cast<float4 *>(row + i) = v;
	}
}

__global__ __launch_bounds__(256) void k_sample_sources(gas_cursor *__restrict__ cursors, const uint32_t *__restrict__ slots, uint32_t n, uint32_t F, const float *__restrict__ fade_env, gas_audio_frame *__restrict__ rows, const uint32_t *__restrict__ row_inc, const uint8_t *__restrict__ feed) {
	const int lane = threadIdx.x & 63;
	const uint32_t e = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (e >= n) {
		return;
	}
	if (feed) { // wave-uniform
		const uint32_t word = reinterpret_cast<const uint32_t *>(feed)[e];
		if (word != GAS_FEED_NONE) {
			fed_row(feed, word, rows + (size_t)e * F, F, lane);
			return;
		}
	}
	gas_cursor *cp = cursors + slots[e];
	const gas_cursor c = *cp;
	const pcm_src src{ c.pcm, c.format_channels >> 8, c.format_channels & 0xff };
	if (src.fmt >= GAS_PCM_IMA_ADPCM) {
		return; // k_sample_adpcm.hip's or k_sample_qoa.hip's row, launched behind this kernel over the same list
	}
	const uint64_t inc = (c.resampled && row_inc) ? row_inc[e] : 65536u;
	gas_sample_row(cp, c, rows + (size_t)e * F, F, lane, inc, fade_env, src);
}

} // namespace

hipError_t gas_launch_sample_sources(hipStream_t stream, gas_cursor *cursors, const uint32_t *slots, uint32_t n, uint32_t frames, const float *fade_env, gas_audio_frame *rows, const uint32_t *row_inc, const uint8_t *feed) {
	if (n == 0) {
		return hipSuccess;
	}
	hipLaunchKernelGGL(k_sample_sources, dim3((n + 3) / 4), dim3(256), 0, stream, cursors, slots, n, frames, fade_env, rows, row_inc, feed);
	return hipGetLastError();
}
