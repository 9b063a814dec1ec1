// gas_qoa.h -- GAS_PCM_QOA (gas_amd.h): the QOA ("Quite OK Audio") file layout, its validator, the dequantisation table,
// the one decoder step and the builder of the records a stream keeps in device memory.  Plain C++ for host and device:
// no HIP runtime call in here, so a stand-alone host program can include it (tests/test_qoa_host_program.py builds one
// under the sanitizers).  The format and the decoder are stated in full in include/gas_amd.h.
//
// Device layout: one 64-byte record per chunk of GAS_QOA_CHUNK = 80 frames (4 slices) and channel, [chunk][channel]:
// the chunk's 4 slices as stored (big-endian, 32 bytes; slices past the stream's end are zero), then the decoder state
// in front of the chunk's first frame (history 4 x int16, weights 4 x int32: inside a QOA frame the weights outgrow 16
// bits on hostile data), then 8 bytes of padding.  A QOA frame is 5120 = 64 x 80 frames, so a chunk never straddles a
// frame header and record idx / 80 holds stream frame idx, at most 80 decoder steps from a known state.  512 bits per 80
// samples: 6.4 bits per sample, one aligned 64-byte line per chunk.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GAS_QOA_HD __host__ __device__
#else
#define GAS_QOA_HD
#endif

#if defined(__HIP_DEVICE_COMPILE__)
extern "C" __device__ int __ockl_mul24_i32(int, int); // the device library's 24-bit multiply (what __mul24 calls)
#endif

#define GAS_QOA_SLICE 20 // frames per slice
#define GAS_QOA_CHUNK 80 // frames per record: 4 slices
#define GAS_QOA_CHUNK_SLICES 4
#define GAS_QOA_FRAME 5120 // frames per QOA frame: 256 slices, 64 chunks
#define GAS_QOA_FRAME_SLICES 256

struct alignas(64) gas_qoa_record {
	uint8_t slices[GAS_QOA_CHUNK_SLICES][8]; // as stored
	int16_t history[4];
	int32_t weights[4];
	uint8_t pad[8];
};
static_assert(sizeof(gas_qoa_record) == 64, "gas_qoa_record layout");

struct gas_qoa_lms {
	int32_t h[4]; // the last four samples, each within int16
	int32_t w[4];
};

GAS_QOA_HD inline uint64_t gas_qoa_chunks(uint64_t frames) {
	return (frames + GAS_QOA_CHUNK - 1) / GAS_QOA_CHUNK;
}
GAS_QOA_HD inline uint64_t gas_qoa_device_bytes(uint64_t frames, uint32_t channels) {
	return gas_qoa_chunks(frames) * channels * sizeof(gas_qoa_record);
}
// fsamples / slices per channel / fsize of QOA frame f of a stream of `frames` frames
GAS_QOA_HD inline uint32_t gas_qoa_frame_samples(uint64_t frames, uint64_t f) {
	const uint64_t left = frames - f * GAS_QOA_FRAME;
	return left < GAS_QOA_FRAME ? (uint32_t)left : GAS_QOA_FRAME;
}
GAS_QOA_HD inline uint32_t gas_qoa_frame_slices(uint32_t fsamples) {
	return (fsamples + GAS_QOA_SLICE - 1) / GAS_QOA_SLICE;
}
GAS_QOA_HD inline uint32_t gas_qoa_frame_bytes(uint32_t fsamples, uint32_t channels) {
	return 8 + 16 * channels + 8 * gas_qoa_frame_slices(fsamples) * channels;
}
// bytes of the whole file: what gas_stream_create reads
GAS_QOA_HD inline uint64_t gas_qoa_file_bytes(uint64_t frames, uint32_t channels) {
	const uint64_t full = frames / GAS_QOA_FRAME;
	const uint32_t rest = (uint32_t)(frames % GAS_QOA_FRAME);
	return 8 + full * gas_qoa_frame_bytes(GAS_QOA_FRAME, channels) + (rest ? gas_qoa_frame_bytes(rest, channels) : 0);
}

GAS_QOA_HD inline uint32_t gas_qoa_be(const uint8_t *p, uint32_t bytes) {
	uint32_t v = 0;
	for (uint32_t i = 0; i < bytes; i++) {
		v = (v << 8) | p[i];
	}
	return v;
}
GAS_QOA_HD inline uint64_t gas_qoa_be64(const uint8_t *p) {
	return ((uint64_t)gas_qoa_be(p, 4) << 32) | gas_qoa_be(p + 4, 4);
}

// DEQ[sf][code] = round-half-away-from-zero of round((sf + 1)^2.75) x {0.75, -0.75, 2.5, -2.5, 4.5, -4.5, 7, -7}[code];
// index sf * 8 + code.
#define GAS_QOA_DEQ_ENTRIES 128
GAS_QOA_HD inline int32_t gas_qoa_dequant(uint32_t i) {
	static constexpr int16_t DEQ[GAS_QOA_DEQ_ENTRIES] = {
		1, -1, 3, -3, 5, -5, 7, -7,
		5, -5, 18, -18, 32, -32, 49, -49,
		16, -16, 53, -53, 95, -95, 147, -147,
		34, -34, 113, -113, 203, -203, 315, -315,
		63, -63, 210, -210, 378, -378, 588, -588,
		104, -104, 345, -345, 621, -621, 966, -966,
		158, -158, 528, -528, 950, -950, 1477, -1477,
		228, -228, 760, -760, 1368, -1368, 2128, -2128,
		316, -316, 1053, -1053, 1895, -1895, 2947, -2947,
		422, -422, 1405, -1405, 2529, -2529, 3934, -3934,
		548, -548, 1828, -1828, 3290, -3290, 5117, -5117,
		696, -696, 2320, -2320, 4176, -4176, 6496, -6496,
		868, -868, 2893, -2893, 5207, -5207, 8099, -8099,
		1064, -1064, 3548, -3548, 6386, -6386, 9933, -9933,
		1286, -1286, 4288, -4288, 7718, -7718, 12005, -12005,
		1536, -1536, 5120, -5120, 9216, -9216, 14336, -14336,
	};
	return DEQ[i];
}

// One decoder step, the only definition of the arithmetic: dequantised residual d moves the state; returns the sample.
// 32-bit two's-complement arithmetic that wraps, written with unsigned operations (the products of hostile weights
// overflow); the shift of the prediction is arithmetic.
GAS_QOA_HD inline int32_t gas_qoa_step(gas_qoa_lms &s, int32_t d) {
	const int32_t delta = d >> 4;
#if defined(__HIP_DEVICE_COMPILE__)
	// The same arithmetic in full-rate 24-bit multiply-adds (the 32-bit multiply runs at a quarter of the rate).  A frame
	// header gives |w| <= 2^15 and a step moves w by |delta| <= 14336 >> 4 = 896, so inside a frame of 5120 samples
	// |w| < 2^15 + 5120 * 896 < 2^23, and |h| <= 2^15: the low 32 bits of the products are the same.  The weight update
	// multiplies delta by the sign (-1 or 1) of its history sample instead of selecting.
	const uint32_t acc = (uint32_t)__ockl_mul24_i32(s.w[0], s.h[0]) + (uint32_t)__ockl_mul24_i32(s.w[1], s.h[1]) + (uint32_t)__ockl_mul24_i32(s.w[2], s.h[2]) + (uint32_t)__ockl_mul24_i32(s.w[3], s.h[3]);
	for (int i = 0; i < 4; i++) {
		s.w[i] = (int32_t)((uint32_t)s.w[i] + (uint32_t)__ockl_mul24_i32((s.h[i] >> 31) | 1, delta));
	}
#else
	const uint32_t acc = (uint32_t)s.w[0] * (uint32_t)s.h[0] + (uint32_t)s.w[1] * (uint32_t)s.h[1] + (uint32_t)s.w[2] * (uint32_t)s.h[2] + (uint32_t)s.w[3] * (uint32_t)s.h[3];
	for (int i = 0; i < 4; i++) {
		s.w[i] = (int32_t)((uint32_t)s.w[i] + (s.h[i] < 0 ? 0u - (uint32_t)delta : (uint32_t)delta));
	}
#endif
	const int32_t p = (int32_t)acc >> 13; // |p| < 2^18: p + d cannot overflow
	int32_t v = p + d;
	v = v < -32768 ? -32768 : v;
	v = v > 32767 ? 32767 : v;
	s.h[0] = s.h[1];
	s.h[1] = s.h[2];
	s.h[2] = s.h[3];
	s.h[3] = v;
	return v;
}

// Residual code k (0 .. 19) of a slice and its scale factor.
GAS_QOA_HD inline uint32_t gas_qoa_slice_sf(uint64_t slice) {
	return (uint32_t)(slice >> 60);
}
GAS_QOA_HD inline uint32_t gas_qoa_slice_code(uint64_t slice, uint32_t k) {
	return (uint32_t)(slice >> (57 - 3 * k)) & 7u;
}

// The sample of frame `last` (< GAS_QOA_CHUNK) of a record's chunk: last + 1 steps from the record's state.  The
// per-load decode of k_sample_qoa.hip and of the stand-alone host program.
GAS_QOA_HD inline int32_t gas_qoa_record_sample(const gas_qoa_record &r, uint32_t last) {
	gas_qoa_lms s;
	for (int i = 0; i < 4; i++) {
		s.h[i] = r.history[i];
		s.w[i] = r.weights[i];
	}
	int32_t v = 0;
	for (uint32_t f0 = 0; f0 <= last; f0 += GAS_QOA_SLICE) {
		const uint64_t slice = gas_qoa_be64(r.slices[f0 / GAS_QOA_SLICE]);
		const uint32_t sf8 = gas_qoa_slice_sf(slice) * 8, n = last - f0 < GAS_QOA_SLICE - 1 ? last - f0 + 1 : GAS_QOA_SLICE;
		for (uint32_t k = 0; k < n; k++) {
			v = gas_qoa_step(s, gas_qoa_dequant(sf8 + gas_qoa_slice_code(slice, k)));
		}
	}
	return v;
}

// True if the `size` bytes at `data` are the QOA file of a stream of `frames` frames and `channels` channels: the magic
// (checked before anything else is read), the sample count, and in every frame header the channel count, fsamples and
// fsize the layout implies.  The sample-rate fields are ignored.
inline bool gas_qoa_validate(const uint8_t *data, uint64_t size, uint32_t channels, uint64_t frames) {
	if (size < 4 || data[0] != 'q' || data[1] != 'o' || data[2] != 'a' || data[3] != 'f') {
		return false;
	}
	if ((channels != 1 && channels != 2) || frames == 0 || frames > 0xffffffffull || size < 8 || gas_qoa_be(data + 4, 4) != frames) {
		return false;
	}
	if (size < gas_qoa_file_bytes(frames, channels)) {
		return false;
	}
	const uint8_t *p = data + 8;
	for (uint64_t f = 0; f * GAS_QOA_FRAME < frames; f++) {
		const uint32_t fsamples = gas_qoa_frame_samples(frames, f), fsize = gas_qoa_frame_bytes(fsamples, channels);
		if (p[0] != channels || gas_qoa_be(p + 4, 2) != fsamples || gas_qoa_be(p + 6, 2) != fsize) {
			return false;
		}
		p += fsize;
	}
	return true;
}

// Fills out[gas_qoa_chunks(frames) * channels], zeroed by the caller, from a validated file: one pass of the decoder,
// every frame header reloading the state (nothing carries across a frame edge).
inline void gas_qoa_build_records(const uint8_t *data, uint32_t channels, uint64_t frames, gas_qoa_record *out) {
	const uint8_t *p = data + 8;
	for (uint64_t f = 0; f * GAS_QOA_FRAME < frames; f++) {
		const uint32_t fsamples = gas_qoa_frame_samples(frames, f), slices = gas_qoa_frame_slices(fsamples);
		for (uint32_t c = 0; c < channels; c++) {
			const uint8_t *st = p + 8 + 16 * c;
			gas_qoa_lms s;
			for (int i = 0; i < 4; i++) {
				s.h[i] = (int16_t)gas_qoa_be(st + 2 * i, 2);
				s.w[i] = (int16_t)gas_qoa_be(st + 8 + 2 * i, 2);
			}
			for (uint32_t k = 0; k < slices; k++) {
				const uint8_t *sl = p + 8 + 16 * channels + 8 * ((size_t)k * channels + c);
				gas_qoa_record &r = out[(f * (GAS_QOA_FRAME / GAS_QOA_CHUNK) + k / GAS_QOA_CHUNK_SLICES) * channels + c];
				if (k % GAS_QOA_CHUNK_SLICES == 0) {
					for (int i = 0; i < 4; i++) {
						r.history[i] = (int16_t)s.h[i];
						r.weights[i] = s.w[i];
					}
				}
				for (int i = 0; i < 8; i++) {
					r.slices[k % GAS_QOA_CHUNK_SLICES][i] = sl[i];
				}
				const uint64_t slice = gas_qoa_be64(sl);
				const uint32_t sf8 = gas_qoa_slice_sf(slice) * 8, left = fsamples - k * GAS_QOA_SLICE;
				for (uint32_t j = 0; j < (left < GAS_QOA_SLICE ? left : GAS_QOA_SLICE); j++) {
					gas_qoa_step(s, gas_qoa_dequant(sf8 + gas_qoa_slice_code(slice, j)));
				}
			}
		}
		p += gas_qoa_frame_bytes(fsamples, channels);
	}
}
