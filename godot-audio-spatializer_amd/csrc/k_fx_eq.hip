// k_fx_eq.hip -- the engine's graphic equalisers as a stage of a staged effect chain (rows in -> dense rows out,
// DESIGN.md 3.5f), gains from gas_fx_eq_settings by chain position, read once per block (no ramp):
//
//   GAS_FX_EQ6 / _EQ10 / _EQ21  [ENGINE] AudioEffectEQInstance::process over EQ::BandProcess.  NOT pinned against the
//     engine's source (a recollection, like the other [ENGINE] kinds).  B bands, each an independent second-order
//     recurrence per ear with coefficients c1, c2, c3 from the context's table (gas_ctx.hip, make_eq_coefs) and the
//     history a2, a3, b2, b3 in the slot's bank; per sample x:
//       b1 = ((c1 (x - a3)) + (c3 b2)) - (c2 b3),   a3 = a2, a2 = x, b3 = b2, b2 = b1
//     and per frame and ear, in band order:  y = 0,  y = y + b1_k g_k,  g_k = db2lin(band_gain_db[k]) once per block
//     (f64 exp, rounded to f32, as k_fx_dyn's db2lin_block).
//
// Geometry (wave64, NT = 256 threads): one lane per (source, band), S = NT / B sources per workgroup (42, 25, 12),
// every lane one recurrence carried for both ears at once: the ears share c1..c3, and explicit two-wide vectors
// (ext_vector_type, lowered to v_pk_mul_f32 / v_pk_add_f32) halve the serial issue; they round exactly like two separate
// f32 operations.  Not scanned: the band poles sit at radius 0.99 .. 0.99994, where scans leave the 1e-5 parity band
// (k_shelf_scan's notes).  The rows are staged through LDS in [S x KF frames] tiles with coalesced 16-byte loads by all
// threads (the next tile's loads in flight during the current one, as k_fx_dyn does), and every tile runs in two passes:
//   1. per lane: the input terms c1 (x_n - x_{n-2}) of the tile's KF frames first (independent of the recurrence), then
//      the recurrence in the engine's order -- per step c3 b2 -> + -> - on the critical path, c2 b3 off it -- with the
//      outputs b1 into LDS ([frame][lane] pairs);
//   2. across all threads, one per (source, frame, ear): the gain-weighted band sum in band order, back into the tile.
// No FMA contraction: the products and sums round like the engine's separate f32 operations.
#include <cmath>

#include "gas_internal.h"

#pragma clang fp contract(off)

namespace {

typedef float f2 __attribute__((ext_vector_type(2))); // (left, right): one packed operation per step for both ears

constexpr int NT = 256; // threads per workgroup
constexpr int KF = 16; // frames per staged tile
constexpr int COLS = KF * 2; // floats of one source per tile (interleaved ears)
constexpr int ROW = COLS + 2; // LDS tile row stride in floats
constexpr int PARTS = COLS / 4; // 16-byte pieces of one source's tile row

template <int B>
struct Geo {
	static constexpr int S = NT / B; // sources per workgroup
	static constexpr int LANES = S * B; // recurrence lanes (the rest idle in pass 1)
	static constexpr int LOADS = (S * PARTS + NT - 1) / NT; // staging loads per thread per tile
	static constexpr int WSTR = 2 * LANES + 2; // LDS stride of one frame's band outputs: pass 2 reads f, ear -> distinct banks
};

__device__ __forceinline__ float db2lin_block(float db) {
	return (float)exp((double)db * 0.11512925464970228);
}

template <int B>
__global__ __launch_bounds__(NT) void k_fx_eq(gas_group_args g, gas_dev_state st, gas_eq_coefs cf, uint32_t F, uint32_t j, float *__restrict__ rows_out) {
	constexpr int S = Geo<B>::S, LANES = Geo<B>::LANES, LOADS = Geo<B>::LOADS, WSTR = Geo<B>::WSTR;
	__shared__ float tile[2][S * ROW];
	__shared__ float work[KF * WSTR];
	__shared__ float gain[LANES];

	const int tid = threadIdx.x;
	const uint32_t e0 = blockIdx.x * S;
	const bool lane_on = tid < LANES;
	const int me = lane_on ? tid / B : 0; // this lane's source within the workgroup and band
	const int band = lane_on ? tid % B : 0;
	const uint32_t e = e0 + me;
	const bool valid = lane_on && e < g.n;
	const uint32_t ec = e < g.n ? e : g.n - 1;
	const uint32_t slot = g.slots ? g.slots[ec] : g.slot_base + ec;
	const int32_t bank = st.eq_of[(size_t)j * st.dyn_stride + slot];
	float *state = valid && bank >= 0 ? st.eq_pool + (size_t)bank * GAS_EQ_BANK_FLOATS + band * 8 : nullptr;

	// block constants and state of this lane's recurrence
	const float c1 = cf.c1[band], c2 = cf.c2[band], c3 = cf.c3[band];
	f2 a2 = { 0.0f, 0.0f }, a3 = a2, b2 = a2, b3 = a2;
	if (state) {
		const float4 h0 = *reinterpret_cast<const float4 *>(state);
		const float4 h1 = *reinterpret_cast<const float4 *>(state + 4);
		a2 = f2{ h0.x, h0.y };
		a3 = f2{ h0.z, h0.w };
		b2 = f2{ h1.x, h1.y };
		b3 = f2{ h1.z, h1.w };
	}
	if (lane_on) {
		gain[tid] = db2lin_block(st.eq_settings[slot].band_gain_db[j][band]);
	}

	// staging: load q of this thread covers source idx / PARTS, 16-byte piece idx % PARTS of the tile (idx = q * NT + tid)
	const float *ld[LOADS];
	float *sto[LOADS];
#pragma unroll
	for (int q = 0; q < LOADS; q++) {
		const int idx = q * NT + tid;
		const uint32_t le = e0 + idx / PARTS;
		const bool in_tile = idx < S * PARTS;
		const uint32_t lc = le < g.n ? le : g.n - 1;
		const uint32_t lrow = g.rows ? g.rows[lc] : lc;
		ld[q] = in_tile ? reinterpret_cast<const float *>(g.src) + (size_t)lrow * F * 2 + (idx % PARTS) * 4 : nullptr;
		sto[q] = in_tile && le < g.n ? rows_out + (size_t)le * F * 2 + (idx % PARTS) * 4 : nullptr;
	}
	float4 pre[LOADS];
#pragma unroll
	for (int q = 0; q < LOADS; q++) {
		if (ld[q]) {
			pre[q] = *reinterpret_cast<const float4 *>(ld[q]);
		}
	}

	const uint32_t n_tiles = F / KF;
	for (uint32_t tl = 0; tl < n_tiles; tl++) {
		float *tb = tile[tl & 1];
#pragma unroll
		for (int q = 0; q < LOADS; q++) { // rows are 136 B apart: two 8-byte stores
			if (ld[q]) {
				const int idx = q * NT + tid;
				float *d = tb + (idx / PARTS) * ROW + (idx % PARTS) * 4;
				*reinterpret_cast<float2 *>(d) = make_float2(pre[q].x, pre[q].y);
				*reinterpret_cast<float2 *>(d + 2) = make_float2(pre[q].z, pre[q].w);
			}
		}
		if (tl + 1 < n_tiles) {
#pragma unroll
			for (int q = 0; q < LOADS; q++) {
				if (ld[q]) {
					pre[q] = *reinterpret_cast<const float4 *>(ld[q] + (size_t)(tl + 1) * COLS);
				}
			}
		}
		__syncthreads();

		// 1. one recurrence per lane: input terms, then the serial steps in the engine's order
		if (lane_on) {
			const float *xr = tb + me * ROW;
			f2 x[KF], u[KF];
#pragma unroll
			for (int k = 0; k < KF; k++) {
				x[k] = f2{ xr[2 * k], xr[2 * k + 1] };
			}
#pragma unroll
			for (int k = 0; k < KF; k++) {
				const f2 xm2 = k >= 2 ? x[k - 2] : (k == 1 ? a2 : a3); // a3 at step k is x_{k-2}
				u[k] = c1 * (x[k] - xm2);
			}
			a2 = x[KF - 1];
			a3 = x[KF - 2];
			float *wp = work + 2 * tid;
#pragma unroll
			for (int k = 0; k < KF; k++) {
				const f2 b1 = (u[k] + c3 * b2) - c2 * b3;
				b3 = b2;
				b2 = b1;
				*reinterpret_cast<float2 *>(wp + k * WSTR) = make_float2(b1.x, b1.y);
			}
		}
		__syncthreads();

		// 2. the gain-weighted band sum, one thread per (source, frame, ear), back into the tile
		for (int idx = tid; idx < S * KF * 2; idx += NT) {
			const int ear = idx & 1, f = (idx >> 1) % KF, s = (idx >> 1) / KF;
			const float *w = work + f * WSTR + 2 * s * B + ear;
			const float *gs = gain + s * B;
			float y = 0.0f;
#pragma unroll
			for (int k = 0; k < B; k++) {
				y = y + w[2 * k] * gs[k];
			}
			tb[s * ROW + 2 * f + ear] = y;
		}
		__syncthreads();

		// rows out with the staging loads' own coalesced pattern
#pragma unroll
		for (int q = 0; q < LOADS; q++) {
			if (sto[q]) {
				const int idx = q * NT + tid;
				const float *t4 = tb + (idx / PARTS) * ROW + (idx % PARTS) * 4;
				*reinterpret_cast<float4 *>(sto[q] + (size_t)tl * COLS) = make_float4(t4[0], t4[1], t4[2], t4[3]);
			}
		}
		// the next tile fills the other buffer; this one is rewritten after the next tile's barriers
	}

	if (state) {
		*reinterpret_cast<float4 *>(state) = make_float4(a2.x, a2.y, a3.x, a3.y);
		*reinterpret_cast<float4 *>(state + 4) = make_float4(b2.x, b2.y, b3.x, b3.y);
	}
}

} // namespace

int gas_eq_bands(int kind) {
	return kind == GAS_FX_EQ6 ? 6 : (kind == GAS_FX_EQ10 ? 10 : (kind == GAS_FX_EQ21 ? 21 : 0));
}

hipError_t gas_launch_fx_eq(hipStream_t stream, int kind, const gas_group_args &g, const gas_dev_state &st, const gas_eq_coefs &coefs, uint32_t frames, uint32_t chain_pos, gas_audio_frame *rows_out) {
	if (g.n == 0) {
		return hipSuccess;
	}
	if (frames % KF != 0 || frames < KF || chain_pos >= GAS_MAX_EFFECTS || !st.eq_pool) {
		return hipErrorInvalidValue;
	}
	float *out = reinterpret_cast<float *>(rows_out);
	switch (kind) {
		case GAS_FX_EQ6:
			hipLaunchKernelGGL(k_fx_eq<6>, dim3((g.n + Geo<6>::S - 1) / Geo<6>::S), dim3(NT), 0, stream, g, st, coefs, frames, chain_pos, out);
			break;
		case GAS_FX_EQ10:
			hipLaunchKernelGGL(k_fx_eq<10>, dim3((g.n + Geo<10>::S - 1) / Geo<10>::S), dim3(NT), 0, stream, g, st, coefs, frames, chain_pos, out);
			break;
		case GAS_FX_EQ21:
			hipLaunchKernelGGL(k_fx_eq<21>, dim3((g.n + Geo<21>::S - 1) / Geo<21>::S), dim3(NT), 0, stream, g, st, coefs, frames, chain_pos, out);
			break;
		default:
			return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
