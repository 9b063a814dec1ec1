// k_conv.hip -- the bus convolvers (gas_conv_*): a long impulse response convolved with a bus mix by uniformly
// partitioned overlap-save, partition length = the callback's F frames.
//
// NEW, with no engine counterpart (the reference mixes buses on the CPU and has no convolution); the rule is the one of
// include/gas_amd.h:   y_e[t] = dry x_e[t] + wet sum_j h_e[j] x_e[t - j].   Checked against tests/conv_ref.py.
//
// One 1024-point real transform serves every legal F (2 F <= 1024): the window of block b is
// [zeros(1024 - 2 F), block b - 1, block b], partition k of the IR sits at the front of its own window, and of the
// circular product the last F outputs are exact (they reach back F - 1 frames, never across the window's start).
// A real 1024-point transform is one fft512 (gas_hrtf_wave.h) of z[n] = w[2 n] + i w[2 n + 1] and an untangling pass:
//   E[k] = (Z[k] + conj Z[512 - k]) / 2,  O[k] = (Z[k] - conj Z[512 - k]) / 2i,  X[k] = E[k] + W1024^k O[k],  X[512] = Re Z[0] - Im Z[0]
// and back:  Z[k] = E[k] + i O[k]  with  E[k] = (Y[k] + conj Y[512 - k]) / 2,  O[k] = W1024^-k (Y[k] - conj Y[512 - k]) / 2.
// A spectrum is bins 0 .. 511 as float2 (4 KiB), the real bin 512 parked in bin 0's imaginary part.
//
// Three launches per call, all over the call's named instances (gas_conv_call, by value):
//   k_conv_forward   one wave per (instance, ear): window -> spectrum -> the instance's ring at this block's position;
//                    this block replaces the previous one (kept per instance and ear next to the ring)
//   k_conv_mac       Y[bin] = sum_k X_{b-k}[bin] H_k[bin] over the partitions the IR has: 256 threads per (instance, ear,
//                    chunk of partitions), a thread owning two bins (16-byte loads, sixteen in flight); the bytes that
//                    matter -- k_ir x 8 KiB per ear -- spread over k_ir / chunk length workgroup rows
//   k_conv_inverse   one workgroup of two waves per instance (wave = ear): chunk sums added in chunk order, back
//                    transform, the last F samples, out = dry in + wet y as 16-byte stores (both ears of two frames)
// A fading instance (gas_conv_fade_to: state A -> state B over N calls) keeps its one input ring and adds
//   k_conv_mac<true>       two more rows behind the call's own: the same walk over the same ring with B's spectra
//                          (skipped where B names A's IR), split into chunks by B's length alone
//   k_conv_inverse_fade    a second launch over the fading instances only, four waves (state x ear): both sums
//                          transformed back side by side, out = (1 - s)(dry_A in + wet_A y^A) + s (dry_B in + wet_B y^B)
// while the settled instances of the call stay on k_conv_inverse; a call without a fade launches what it always did.
// A four-channel ("true stereo") IR, y_e = dry x_e + wet sum_j (h_0e[j] x_0[t - j] + h_1e[j] x_1[t - j]), changes the
// middle launch only: a call that names one anywhere launches
//   k_conv_mac_ts          in place of k_conv_mac<>: a true-stereo row reads both ears' rings and two channels' spectra
//                          (a direct and a cross accumulator, added once per chunk); every other row, state B's included,
//                          runs the walk above with the bits above
// and a call that names none launches what it always did.  Rings, partial sums and the inverse stages are the same.
// Vector stores only, no atomics; every sum has a fixed order, so two runs give the same bits.
#include "gas_hrtf_wave.h"

#include <cmath>

namespace {

__device__ __forceinline__ void conv_twiddles(const float2 *__restrict__ tw, int lane, float2 (&t1)[8], float2 (&t2)[8]) {
#pragma unroll
	for (int k = 0; k < 8; k++) {
		t1[k] = tw[k * 64 + lane];
		t2[k] = tw[(8 + k) * 64 + lane];
	}
}

// v[j] = z[lane + 64 j] of a packed real window -> dst[lane + 64 j] = scale * X[lane + 64 j]
__device__ __forceinline__ void conv_spectrum(float2 (&v)[8], const float2 (&t1)[8], const float2 (&t2)[8], float2 *lds, int lane, const float2 *__restrict__ w1024, float scale, float2 *__restrict__ dst) {
	fft512<false>(v, t1, t2, lds, lane);
#pragma unroll
	for (int j = 0; j < 8; j++) {
		lds[lane + 64 * j] = v[j];
	}
	wave_lds_sync();
#pragma unroll
	for (int j = 0; j < 8; j++) {
		const int k = lane + 64 * j;
		const float2 m = lds[(512 - k) & 511];
		const float2 w = w1024[k];
		const float2 e = make_float2(0.5f * (v[j].x + m.x), 0.5f * (v[j].y - m.y));
		const float2 o = make_float2(0.5f * (v[j].y + m.y), -0.5f * (v[j].x - m.x)); // (Z - conj Zm) / 2i
		float2 x = cadd(e, cmul(w, o));
		if (k == 0) {
			x = make_float2(v[0].x + v[0].y, v[0].x - v[0].y); // bins 0 and 512, both real
		}
		dst[k] = make_float2(scale * x.x, scale * x.y);
	}
}

__global__ __launch_bounds__(64) void k_conv_forward(gas_conv_call call, gas_conv_pool pool, const float2 *__restrict__ tw, const gas_audio_frame *__restrict__ in, uint32_t F) {
	__shared__ float2 lds[LDS_F2_HALF];
	const int lane = threadIdx.x;
	const uint32_t i = blockIdx.x >> 1, ear = blockIdx.x & 1;
	const gas_conv_entry en = call.e[i];
	const int SQ = (int)(F / 128); // a block is SQ registers of 64 sample pairs
	float2 t1[8], t2[8];
	conv_twiddles(tw, lane, t1, t2);
	// Pair q of the previous block and pair q of this one belong to the same lane (registers SQ apart), so the lane that
	// reads a pair of `prev` is the one that replaces it, in program order.
	float *prev = pool.prev + (size_t)(en.slot * 2 + ear) * 512;
	const float4 *row = reinterpret_cast<const float4 *>(in + (size_t)i * F); // two frames: L0 R0 L1 R1
	float2 v[8];
#pragma unroll
	for (int j = 0; j < 8; j++) {
		const int jj = j - (8 - 2 * SQ);
		if (jj < 0) {
			v[j] = make_float2(0.0f, 0.0f);
		} else if (jj < SQ) {
			v[j] = *reinterpret_cast<const float2 *>(prev + 2 * (lane + 64 * jj));
		} else {
			const int q = lane + 64 * (jj - SQ);
			const float4 f = row[q];
			v[j] = ear ? make_float2(f.y, f.w) : make_float2(f.x, f.z);
			*reinterpret_cast<float2 *>(prev + 2 * q) = v[j];
		}
	}
	float2 *dst = pool.ring + ((size_t)(en.slot * 2 + ear) * pool.K + en.pos) * GAS_CONV_BINS;
	conv_spectrum(v, t1, t2, lds, lane, pool.w1024, 1.0f, dst);
}

// IR [channels][taps] -> H[channel][partition][512]: partition k's F taps at the front of a zero window, scaled by
// 1/512 so that the inverse stage needs no normalisation (k_hrtf_table does the same for the HRIRs).
__global__ __launch_bounds__(64) void k_conv_ir(const float *__restrict__ ir, uint32_t taps, uint32_t k_ir, uint32_t F, const float2 *__restrict__ tw, const float2 *__restrict__ w1024, float2 *__restrict__ H) {
	__shared__ float2 lds[LDS_F2_HALF];
	const int lane = threadIdx.x;
	const uint32_t ch = blockIdx.x / k_ir, k = blockIdx.x % k_ir;
	float2 t1[8], t2[8];
	conv_twiddles(tw, lane, t1, t2);
	const float *h = ir + (size_t)ch * taps;
	float2 v[8];
#pragma unroll
	for (int j = 0; j < 8; j++) {
		const uint32_t s = 2u * (uint32_t)(lane + 64 * j); // window index of the pair
		const uint32_t t = k * F + s; // tap index
		v[j] = make_float2(s < F && t < taps ? h[t] : 0.0f, s + 1 < F && t + 1 < taps ? h[t + 1] : 0.0f);
	}
	conv_spectrum(v, t1, t2, lds, lane, w1024, 1.0f / 512.0f, H + (size_t)blockIdx.x * GAS_CONV_BINS);
}

// acc += x * h for the two bins of a float4; the first thread's first "bin" is the packed pair of real bins 0 and 512
__device__ __forceinline__ void conv_mac(float4 &acc, const float4 x, const float4 h, bool packed) {
	float2 a = make_float2(acc.x, acc.y), b = make_float2(acc.z, acc.w);
	if (packed) {
		a.x = __builtin_fmaf(x.x, h.x, a.x);
		a.y = __builtin_fmaf(x.y, h.y, a.y);
	} else {
		cmac_fixed(a, make_float2(x.x, x.y), h.x, h.y);
	}
	cmac_fixed(b, make_float2(x.z, x.w), h.z, h.w);
	acc = make_float4(a.x, a.y, b.x, b.y);
}

// One workgroup's chunk of the sum over an IR (spectra Hs, k_ir partitions) for one ear of the instance in `slot`, into
// row `row` of the call's partial sums.  The chunk split is a function of k_ir alone.
__device__ __forceinline__ void conv_mac_chunk(const gas_conv_pool &pool, const float2 *__restrict__ Hs, uint32_t k_ir, uint32_t mode, uint32_t slot, uint32_t pos, uint32_t ear, uint32_t row) {
	const uint32_t len = gas_conv_chunk_len(k_ir);
	const uint32_t k0 = blockIdx.x * len;
	if (k0 >= k_ir) { // this IR has fewer chunks than the call's longest
		return;
	}
	const uint32_t k1 = k0 + len < k_ir ? k0 + len : k_ir;
	const uint32_t K = pool.K;
	const float4 *X = reinterpret_cast<const float4 *>(pool.ring + (size_t)(slot * 2 + ear) * K * GAS_CONV_BINS) + threadIdx.x;
	const float4 *H = reinterpret_cast<const float4 *>(Hs + (size_t)(ear & mode) * k_ir * GAS_CONV_BINS) + threadIdx.x; // mono or stereo
	constexpr uint32_t ROW = GAS_CONV_BINS / 2; // float4 per spectrum
	const bool packed = threadIdx.x == 0;
	float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	uint32_t k = k0;
	// partition k meets the spectrum of k blocks ago: ring position pos - k, modulo K
	auto ring_row = [&](uint32_t kk) { return (size_t)(pos >= kk ? pos - kk : pos + K - kk) * ROW; };
	constexpr int U = 8; // partitions per trip: sixteen 16-byte loads in flight per thread
	for (; k + U <= k1; k += U) {
		float4 x[U], h[U];
#pragma unroll
		for (int u = 0; u < U; u++) {
			x[u] = X[ring_row(k + u)];
			h[u] = H[(size_t)(k + u) * ROW];
		}
#pragma unroll
		for (int u = 0; u < U; u++) {
			conv_mac(acc, x[u], h[u], packed);
		}
	}
	for (; k < k1; k++) {
		conv_mac(acc, X[ring_row(k)], H[(size_t)k * ROW], packed);
	}
	reinterpret_cast<float4 *>(pool.ypart + ((size_t)row * pool.max_chunks + blockIdx.x) * GAS_CONV_BINS)[threadIdx.x] = acc;
}

// FADE (a call that names a fading instance): behind the call's own `rows` rows come two per fading entry, the sum over
// state B's IR -- the same walk over the same ring, so after the fade the bits are those of a hard switch to B.
template <bool FADE>
__global__ __launch_bounds__(256) void k_conv_mac(gas_conv_call call, gas_conv_pool pool, uint32_t rows) {
	const uint32_t ie = blockIdx.y, ear = ie & 1;
	if (FADE && ie >= rows) {
		const uint32_t i = call.fading[(ie - rows) >> 1];
		const gas_conv_entry en = call.e[i];
		if (en.HB) { // a level-only fade has no second sum
			conv_mac_chunk(pool, en.HB, en.k_irB, en.modeB, en.slot, en.pos, ear, 2 * GAS_MAX_CONVOLVERS + i * 2 + ear);
		}
		return;
	}
	const gas_conv_entry en = call.e[ie >> 1];
	conv_mac_chunk(pool, en.H, en.k_ir, en.mode, en.slot, en.pos, ear, ie);
}

// TRUE STEREO (an IR of four channels, c = 2 i + e from input ear i to output ear e): the same row and the same chunk
// split, but output ear `ear` walks both ears' rings.  The direct term (input ear `ear`) is conv_mac_chunk's sum, FMA for
// FMA, in one accumulator; the cross term (the other input ear) goes ascending k into a second one; the chunk's sum is
// direct + cross, one add per component.  Four loads per partition, so four partitions per trip keep conv_mac_chunk's
// sixteen 16-byte loads in flight, and the two accumulators are two independent FMA chains.
__device__ __forceinline__ void conv_mac_chunk_ts(const gas_conv_pool &pool, const float2 *__restrict__ Hs, uint32_t k_ir, uint32_t slot, uint32_t pos, uint32_t ear, uint32_t row) {
	const uint32_t len = gas_conv_chunk_len(k_ir);
	const uint32_t k0 = blockIdx.x * len;
	if (k0 >= k_ir) {
		return;
	}
	const uint32_t k1 = k0 + len < k_ir ? k0 + len : k_ir;
	const uint32_t K = pool.K;
	const size_t ring = (size_t)K * GAS_CONV_BINS, chan = (size_t)k_ir * GAS_CONV_BINS;
	const float4 *Xd = reinterpret_cast<const float4 *>(pool.ring + (size_t)(slot * 2 + ear) * ring) + threadIdx.x;
	const float4 *Xc = reinterpret_cast<const float4 *>(pool.ring + (size_t)(slot * 2 + (ear ^ 1)) * ring) + threadIdx.x;
	const float4 *Hd = reinterpret_cast<const float4 *>(Hs + (size_t)(2 * ear + ear) * chan) + threadIdx.x;
	const float4 *Hc = reinterpret_cast<const float4 *>(Hs + (size_t)(2 * (ear ^ 1) + ear) * chan) + threadIdx.x;
	constexpr uint32_t ROW = GAS_CONV_BINS / 2;
	const bool packed = threadIdx.x == 0;
	float4 direct = make_float4(0.0f, 0.0f, 0.0f, 0.0f), cross = direct;
	uint32_t k = k0;
	auto ring_row = [&](uint32_t kk) { return (size_t)(pos >= kk ? pos - kk : pos + K - kk) * ROW; };
	constexpr int U = 4;
	for (; k + U <= k1; k += U) {
		float4 xd[U], xc[U], hd[U], hc[U];
#pragma unroll
		for (int u = 0; u < U; u++) {
			const size_t r = ring_row(k + u), p = (size_t)(k + u) * ROW;
			xd[u] = Xd[r];
			xc[u] = Xc[r];
			hd[u] = Hd[p];
			hc[u] = Hc[p];
		}
#pragma unroll
		for (int u = 0; u < U; u++) {
			conv_mac(direct, xd[u], hd[u], packed);
			conv_mac(cross, xc[u], hc[u], packed);
		}
	}
	for (; k < k1; k++) {
		const size_t r = ring_row(k), p = (size_t)k * ROW;
		conv_mac(direct, Xd[r], Hd[p], packed);
		conv_mac(cross, Xc[r], Hc[p], packed);
	}
	reinterpret_cast<float4 *>(pool.ypart + ((size_t)row * pool.max_chunks + blockIdx.x) * GAS_CONV_BINS)[threadIdx.x] = make_float4(direct.x + cross.x, direct.y + cross.y, direct.z + cross.z, direct.w + cross.w);
}

// The form a call launches when one of its entries names a four-channel IR, as state A or B: rows of one- and
// two-channel IRs run conv_mac_chunk, so their bits are k_conv_mac's.  Rows past `rows` are the fading entries' state B.
__global__ __launch_bounds__(256) void k_conv_mac_ts(gas_conv_call call, gas_conv_pool pool, uint32_t rows) {
	const uint32_t ie = blockIdx.y, ear = ie & 1;
	const bool stateB = ie >= rows;
	const uint32_t i = stateB ? call.fading[(ie - rows) >> 1] : ie >> 1;
	const gas_conv_entry en = call.e[i];
	if (stateB && !en.HB) { // a level-only fade has no second sum
		return;
	}
	const float2 *Hs = stateB ? en.HB : en.H;
	const uint32_t k_ir = stateB ? en.k_irB : en.k_ir, mode = stateB ? en.modeB : en.mode;
	const uint32_t row = stateB ? 2 * GAS_MAX_CONVOLVERS + i * 2 + ear : ie;
	if (mode == GAS_CONV_TRUE_STEREO) { // uniform over the workgroup
		conv_mac_chunk_ts(pool, Hs, k_ir, en.slot, en.pos, ear, row);
	} else {
		conv_mac_chunk(pool, Hs, k_ir, mode, en.slot, en.pos, ear, row);
	}
}

// One wave's share of the inverse stage: `chunks` partial sums from yp added in chunk order, untangled and transformed
// back; the window's last F samples land in y[0 .. F).
__device__ __forceinline__ void conv_back(const float2 *__restrict__ yp, uint32_t chunks, const float2 *__restrict__ w1024, const float2 (&t1)[8], const float2 (&t2)[8], float2 *lds, int lane, int SQ, float *y) {
	float2 a[8], b[8]; // Y[k] and Y[512 - k], k = lane + 64 j
#pragma unroll
	for (int j = 0; j < 8; j++) {
		a[j] = make_float2(0.0f, 0.0f);
	}
	// chunk order; four chunks' loads (32 of 8 bytes) in flight per trip
	uint32_t c = 0;
	for (; c + 4 <= chunks; c += 4) {
		float2 t[4][8];
#pragma unroll
		for (int u = 0; u < 4; u++) {
#pragma unroll
			for (int j = 0; j < 8; j++) {
				t[u][j] = yp[(size_t)(c + u) * GAS_CONV_BINS + lane + 64 * j];
			}
		}
#pragma unroll
		for (int u = 0; u < 4; u++) {
#pragma unroll
			for (int j = 0; j < 8; j++) {
				a[j] = cadd(a[j], t[u][j]);
			}
		}
	}
	for (; c < chunks; c++) {
#pragma unroll
		for (int j = 0; j < 8; j++) {
			a[j] = cadd(a[j], yp[(size_t)c * GAS_CONV_BINS + lane + 64 * j]);
		}
	}
	// the mirrored bins come from the other lanes through the wave's LDS slice
#pragma unroll
	for (int j = 0; j < 8; j++) {
		lds[lane + 64 * j] = a[j];
	}
	wave_lds_sync();
#pragma unroll
	for (int j = 0; j < 8; j++) {
		b[j] = lds[(512 - (lane + 64 * j)) & 511];
	}
	wave_lds_sync();
	float2 v[8];
#pragma unroll
	for (int j = 0; j < 8; j++) {
		const int k = lane + 64 * j;
		const float2 w = w1024[k];
		const float2 e = make_float2(0.5f * (a[j].x + b[j].x), 0.5f * (a[j].y - b[j].y));
		const float2 d = make_float2(0.5f * (a[j].x - b[j].x), 0.5f * (a[j].y + b[j].y));
		const float2 o = cmulc(d, w); // W1024^-k d
		v[j] = make_float2(e.x - o.y, e.y + o.x);
		if (k == 0) { // Y[0] and Y[512] are real, packed into one entry
			v[j] = make_float2(0.5f * (a[0].x + a[0].y), 0.5f * (a[0].x - a[0].y));
		}
	}
	fft512<true>(v, t1, t2, lds, lane);
	// z[n] = y[2 n] + i y[2 n + 1]; the block is the window's last F samples: registers 8 - SQ .. 7
#pragma unroll
	for (int j = 0; j < 8; j++) {
		const int jj = j - (8 - SQ);
		if (jj >= 0) {
			*reinterpret_cast<float2 *>(&y[2 * (lane + 64 * jj)]) = v[j];
		}
	}
}

// The settled instances of a call; a fading one is k_conv_inverse_fade's.
__global__ __launch_bounds__(128) void k_conv_inverse(gas_conv_call call, gas_conv_pool pool, const float2 *__restrict__ tw, const gas_audio_frame *in, gas_audio_frame *out, uint32_t F) {
	__shared__ float2 lds_all[2 * LDS_F2_HALF];
	__shared__ float y[2][512];
	const int lane = threadIdx.x & 63;
	const int ear = threadIdx.x >> 6;
	const uint32_t i = blockIdx.x;
	const gas_conv_entry en = call.e[i];
	if (en.fade_inv != 0.0f) {
		return;
	}
	const int SQ = (int)(F / 128);
	float2 t1[8], t2[8];
	conv_twiddles(tw, lane, t1, t2);
	const float2 *yp = pool.ypart + (size_t)(i * 2 + ear) * pool.max_chunks * GAS_CONV_BINS;
	conv_back(yp, gas_conv_chunks(en.k_ir), pool.w1024, t1, t2, lds_all + ear * LDS_F2_HALF, lane, SQ, y[ear]);
	__syncthreads();
	const float4 *irow = reinterpret_cast<const float4 *>(in + (size_t)i * F);
	float4 *orow = reinterpret_cast<float4 *>(out + (size_t)i * F);
	for (uint32_t q = threadIdx.x; q < F / 2; q += 128) { // frames 2 q and 2 q + 1; out may be in: a thread reads what it writes
		const float4 x = irow[q];
		const float2 yl = *reinterpret_cast<const float2 *>(&y[0][2 * q]);
		const float2 yr = *reinterpret_cast<const float2 *>(&y[1][2 * q]);
		orow[q] = make_float4(en.dry * x.x + en.wet * yl.x, en.dry * x.y + en.wet * yr.x, en.dry * x.z + en.wet * yl.y, en.dry * x.w + en.wet * yr.y);
	}
}

// The fading instances of a call, one workgroup of four waves each: waves 0 and 1 transform state A's sums back (one ear
// each), waves 2 and 3 state B's, at the same time; then frame i is (1 - s) (dry_A x + wet_A y^A) + s (dry_B x + wet_B y^B)
// with s = (float)(fade_t0 + i) * fade_inv.  In a level-only fade y^B is y^A and waves 2 and 3 only take part in the lerp.
__global__ __launch_bounds__(256) void k_conv_inverse_fade(gas_conv_call call, gas_conv_pool pool, const float2 *__restrict__ tw, const gas_audio_frame *in, gas_audio_frame *out, uint32_t F) {
	__shared__ float2 lds_all[4 * LDS_F2_HALF];
	__shared__ float y[4][512]; // [state * 2 + ear]
	const int lane = threadIdx.x & 63;
	const int wave = threadIdx.x >> 6, ear = wave & 1, state = wave >> 1;
	const uint32_t i = call.fading[blockIdx.x];
	const gas_conv_entry en = call.e[i];
	const bool own = en.HB != nullptr; // B has a wet sum of its own
	if (state == 0 || own) { // uniform over a wave
		float2 t1[8], t2[8];
		conv_twiddles(tw, lane, t1, t2);
		const uint32_t row = state * 2 * GAS_MAX_CONVOLVERS + i * 2 + ear;
		const float2 *yp = pool.ypart + (size_t)row * pool.max_chunks * GAS_CONV_BINS;
		conv_back(yp, gas_conv_chunks(state ? en.k_irB : en.k_ir), pool.w1024, t1, t2, lds_all + wave * LDS_F2_HALF, lane, (int)(F / 128), y[wave]);
	}
	__syncthreads();
	const float *ybl = own ? y[2] : y[0], *ybr = own ? y[3] : y[1];
	const float4 *irow = reinterpret_cast<const float4 *>(in + (size_t)i * F);
	float4 *orow = reinterpret_cast<float4 *>(out + (size_t)i * F);
	for (uint32_t q = threadIdx.x; q < F / 2; q += 256) { // frames 2 q and 2 q + 1; out may be in: a thread reads what it writes
		const float4 x = irow[q];
		const float2 al = *reinterpret_cast<const float2 *>(&y[0][2 * q]);
		const float2 ar = *reinterpret_cast<const float2 *>(&y[1][2 * q]);
		const float2 bl = *reinterpret_cast<const float2 *>(&ybl[2 * q]);
		const float2 br = *reinterpret_cast<const float2 *>(&ybr[2 * q]);
		const float s0 = (float)(en.fade_t0 + 2 * q) * en.fade_inv, s1 = (float)(en.fade_t0 + 2 * q + 1) * en.fade_inv;
		const float r0 = 1.0f - s0, r1 = 1.0f - s1;
		orow[q] = make_float4(r0 * (en.dry * x.x + en.wet * al.x) + s0 * (en.dryB * x.x + en.wetB * bl.x), r0 * (en.dry * x.y + en.wet * ar.x) + s0 * (en.dryB * x.y + en.wetB * br.x),
				r1 * (en.dry * x.z + en.wet * al.y) + s1 * (en.dryB * x.z + en.wetB * bl.y), r1 * (en.dry * x.w + en.wet * ar.y) + s1 * (en.dryB * x.w + en.wetB * br.y));
	}
}

} // namespace

void gas_make_w1024(float2 *host_w) {
	const double pi = 3.14159265358979323846264338328;
	for (int k = 0; k < 512; k++) {
		const double a = -pi * (double)k / 512.0;
		host_w[k] = make_float2((float)cos(a), (float)sin(a));
	}
}

hipError_t gas_launch_conv_ir(hipStream_t stream, const float *d_ir, uint32_t channels, uint32_t taps, uint32_t frames, const float2 *twiddles, const float2 *w1024, float2 *H) {
	const uint32_t k_ir = (taps + frames - 1) / frames;
	hipLaunchKernelGGL(k_conv_ir, dim3(channels * k_ir), dim3(64), 0, stream, d_ir, taps, k_ir, frames, twiddles, w1024, H);
	return hipGetLastError();
}

hipError_t gas_launch_conv(hipStream_t stream, gas_conv_call &call, uint32_t n, const gas_conv_pool &pool, const float2 *twiddles, const gas_audio_frame *in, gas_audio_frame *out, uint32_t frames) {
	if (n == 0) {
		return hipSuccess;
	}
	uint32_t chunks = 1, fading = 0;
	bool true_stereo = false; // an entry names a four-channel IR, as state A or as a state B with a sum of its own
	for (uint32_t i = 0; i < n; i++) {
		const gas_conv_entry &en = call.e[i];
		uint32_t c = gas_conv_chunks(en.k_ir);
		true_stereo |= en.mode == GAS_CONV_TRUE_STEREO;
		if (en.fade_inv != 0.0f) {
			call.fading[fading++] = (uint8_t)i;
			const uint32_t cb = en.HB ? gas_conv_chunks(en.k_irB) : 0;
			c = cb > c ? cb : c;
			true_stereo |= en.HB && en.modeB == GAS_CONV_TRUE_STEREO;
		}
		chunks = c > chunks ? c : chunks;
	}
	hipLaunchKernelGGL(k_conv_forward, dim3(n * 2), dim3(64), 0, stream, call, pool, twiddles, in, frames);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) {
		return e;
	}
	if (true_stereo) {
		hipLaunchKernelGGL(k_conv_mac_ts, dim3(chunks, (n + fading) * 2), dim3(256), 0, stream, call, pool, n * 2);
	} else if (fading == 0) {
		hipLaunchKernelGGL(k_conv_mac<false>, dim3(chunks, n * 2), dim3(256), 0, stream, call, pool, n * 2);
	} else {
		hipLaunchKernelGGL(k_conv_mac<true>, dim3(chunks, (n + fading) * 2), dim3(256), 0, stream, call, pool, n * 2);
	}
	e = hipGetLastError();
	if (e != hipSuccess) {
		return e;
	}
	if (fading < n) {
		hipLaunchKernelGGL(k_conv_inverse, dim3(n), dim3(128), 0, stream, call, pool, twiddles, in, out, frames);
		e = hipGetLastError();
		if (e != hipSuccess) {
			return e;
		}
	}
	if (fading > 0) {
		hipLaunchKernelGGL(k_conv_inverse_fade, dim3(fading), dim3(256), 0, stream, call, pool, twiddles, in, out, frames);
		e = hipGetLastError();
	}
	return e;
}
