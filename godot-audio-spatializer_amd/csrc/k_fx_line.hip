// k_fx_line.hip -- the engine's delay and reverb as stages of a staged effect chain (rows in -> dense rows out,
// DESIGN.md 3.5e).  Settings from gas_fx_line_settings by chain position, read once per block; state and delay memory
// in one "line" per effect instance, from the pools of gas_ctx_reserve_fx_lines (addressed through st.line_of).
// The semantics are a recollection of the engine's audio_effect_delay.cpp, reverb_filter.cpp and
// audio_effect_reverb.cpp, not pinned against its source (like SURVEY Appendix B).  Block constants are computed in
// f64 and rounded to f32; db2lin and undenormalize are k_fx_dyn.hip's.
//
//   GAS_FX_DELAY  ears independent, sr the mix rate.  Block constants:
//       D1 = (int)(tap1_ms / 1000 sr), D2 likewise, l1 = tap1_active ? db2lin(tap1_level_db) : 0,
//       v1 = (l1 clamp(1 - pan1, 0, 1), l1 clamp(1 + pan1, 0, 1)), tap 2 likewise, fl = fb_active ? db2lin(fb_level_db) : 0,
//       Dfb = (int)(fb_ms / 1000 sr), c = exp(-2 pi lowpass_hz / sr), ic = 1 - c
//     per frame and ear, state ring (write position P), fb (position q), h:
//       ring[P & mask] = x
//       out = ((x dry + ring[(P - D1) & mask] v1) + ring[(P - D2) & mask] v2) + fb[q]
//       fbin = undenorm((out fl) ic + h c),  h = fbin,  fb[q] = fbin,  y = out,  P += 1,  if (++q >= Dfb) q = 0
//   GAS_FX_REVERB  a mono Reverb per ear (extra spread 0 s / 0.000521 s), lengths fixed per context (gas_line_geo).
//     Block constants: pd = clamp(lrint(predelay_ms / 1000 sr), 10, echo_size - 1), fbk = clamp(0.7 + room 0.28, 0.7, 0.98),
//       auxdmp = (float)(damping / 2 + 0.5), auxdmp *= auxdmp, damp = exp(-2 pi auxdmp 10000 / sr),
//       limit = size - lrintf(xs (1 - spread)) for every comb and allpass,
//       hipass > 0: hpaux = exp(-2 pi hipass 6000 / sr), a1 = (1 + hpaux) / 2, a2 = -a1, b1 = hpaux
//     per block (every position wraps to 0 when it is >= its size / limit, checked before each use):
//       1. in = undenorm(echo[epos - pd] pfb + x), echo[epos] = in, u = in
//       2. hipass > 0 only: v = u, u = v a1 + h1 a2 + h2 b1, h2 = u, h1 = v
//       3. d = 0; combs k = 0..7: o = undenorm(buf[pos] fbk), o = o (1.0 - damp) + dh damp (f64 sum, first product
//          f64), dh = o, buf[pos] = u + o, d += o
//       4. allpasses k = 0..3: aux = buf[pos], buf[pos] = undenorm(0.7 aux + d), d = aux - 0.7 buf[pos]
//       5. y = ((d wet) 0.6) + x dry
//
// Mapping (parallel work on every wave, a serial lane only for what is recurrent):
//   delay: KFD-frame tiles of DS sources; per tile (1) all waves stage x and write the ring, (2) all waves read both
//     taps and, where the previous writer of fb[q] lies before the tile, fb[q] -- coalesced over frames -- (3) one lane
//     of wave 0 per (source, ear) runs the h chain (and, when Dfb < KFD, reads this tile's own fb values from LDS),
//     (4) all waves write the rows and the last fb value per position.  Ring reads never meet this block's later
//     writes: the ring is longer than the longest tap by more than a block.
//   reverb: RS sources (2 RS mono reverbs) per workgroup, the block's u and d in LDS.  Step 1 is parallel (every read
//     before any write: pd >= F, and pd = echo_size - 1 reads what the next frame overwrites), step 2 one lane per
//     reverb, step 3 one lane per comb over KFR-frame tiles whose reads all precede the block's writes (limit >= F),
//     the comb outputs summed in comb order by a parallel pass, step 4 parallel over frames in rounds of `limit`
//     frames (the frames of a round touch distinct positions), step 5 parallel.
// No FMA contraction: products and sums round like the engine's separate f32 operations.
#include <cmath>

#include "gas_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr double TWO_PI = 6.283185307179586;

__device__ __forceinline__ float undenormalize(float v) { // [ENGINE] undenormalize: biased exponent < 16 -> 0
	return (__float_as_uint(v) & 0x7f800000u) < 0x08000000u ? 0.0f : v;
}

__device__ __forceinline__ float db2lin_block(float db) {
	return (float)exp((double)db * 0.11512925464970228);
}

__device__ __forceinline__ double clamp01(double v) {
	return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}

// ---------------------------------------------------------------------------------------------------------------
// GAS_FX_DELAY
// ---------------------------------------------------------------------------------------------------------------
constexpr int DS = 32; // sources per workgroup: wave 0's lane = (source, ear)
constexpr int KFD = 64; // frames per tile
constexpr int DNT = 512; // 8 waves
constexpr int DCOLS = KFD * 2;
constexpr int DROW = DCOLS + 2; // LDS row stride in floats: serial lane (s, ear) reads bank (2 s + ear + 2 k) % 32
constexpr int DPER = DS * DCOLS / DNT; // elements per thread and tile

struct DelaySrc { // per source, LDS
	float dry, v1[2], v2[2];
	int d1, d2, lc, start, q0;
	uint32_t p0;
	float *line; // nullptr: no source, or no line entered (never expected; its rows are written as zeros)
	uint32_t row;
	int out; // a group entry: its rows are written
};

__device__ __forceinline__ int delay_q(int i, int q0, int lc, int start) { // q of frame i of the block
	return i < start ? q0 : (start ? (i - 1) % lc : (q0 + i) % lc);
}

__global__ __launch_bounds__(DNT) void k_fx_delay(gas_group_args g, gas_dev_state st, gas_line_geo geo, uint32_t F, uint32_t j, float mix_rate, float *__restrict__ rows_out) {
	__shared__ DelaySrc src[DS];
	__shared__ float wo[DS * DROW]; // per tile: out (or the sum without fb[q] when its writer is in this tile)
	__shared__ float fbt[DS * DROW]; // per tile: fbin

	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t e0 = blockIdx.x * DS;
	const size_t stride = st.dyn_stride;
	const uint32_t mask = geo.ring_mask;

	// block constants; wave 0's lane (s, ear) keeps its recurrence's in registers
	float fl = 0.0f, c = 0.0f, ic = 0.0f, h = 0.0f;
	int lc = 1, start = 0;
	float *line = nullptr;
	if (wave == 0) {
		const int s = lane >> 1, ear = lane & 1;
		const uint32_t e = e0 + s;
		const uint32_t slot = e < g.n ? (g.slots ? g.slots[e] : g.slot_base + e) : 0;
		const int li = e < g.n ? st.line_of[(size_t)j * stride + slot] : -1; // (-1: no line entered; never expected)
		if (li >= 0) {
			const gas_fx_line_settings *P = st.line_settings + slot;
			line = st.delay_pool + (size_t)li * geo.delay_floats;
			const double sr = (double)mix_rate;
			const uint32_t *hdr = reinterpret_cast<const uint32_t *>(line);
			const int q0 = (int)hdr[1];
			const int dfb = (int)((double)P->delay_feedback_ms[j] / 1000.0 * sr);
			lc = dfb > 1 ? dfb : 1;
			start = q0 >= lc ? 1 : 0;
			fl = P->delay_feedback_active[j] ? db2lin_block(P->delay_feedback_level_db[j]) : 0.0f;
			c = (float)exp(-TWO_PI * (double)P->delay_feedback_lowpass_hz[j] / sr);
			ic = 1.0f - c;
			h = __uint_as_float(hdr[2 + ear]);
			if (ear == 0) {
				DelaySrc d;
				d.dry = P->delay_dry[j];
				const float l1 = P->delay_tap1_active[j] ? db2lin_block(P->delay_tap1_level_db[j]) : 0.0f;
				const float l2 = P->delay_tap2_active[j] ? db2lin_block(P->delay_tap2_level_db[j]) : 0.0f;
				const double pan1 = (double)P->delay_tap1_pan[j], pan2 = (double)P->delay_tap2_pan[j];
				d.v1[0] = (float)((double)l1 * clamp01(1.0 - pan1));
				d.v1[1] = (float)((double)l1 * clamp01(1.0 + pan1));
				d.v2[0] = (float)((double)l2 * clamp01(1.0 - pan2));
				d.v2[1] = (float)((double)l2 * clamp01(1.0 + pan2));
				d.d1 = (int)((double)P->delay_tap1_ms[j] / 1000.0 * sr);
				d.d2 = (int)((double)P->delay_tap2_ms[j] / 1000.0 * sr);
				d.lc = lc;
				d.start = start;
				d.q0 = q0;
				d.p0 = hdr[0];
				d.line = line;
				d.row = g.rows ? g.rows[e] : e;
				d.out = 1;
				src[s] = d;
			}
		} else if ((lane & 1) == 0) {
			src[s].line = nullptr;
			src[s].out = e < g.n;
		}
	}
	__syncthreads();

	for (uint32_t t0 = 0; t0 < F; t0 += KFD) {
		// 1. stage x and write the ring
		float x[DPER];
#pragma unroll
		for (int q = 0; q < DPER; q++) {
			const int idx = q * DNT + tid;
			const int s = idx / DCOLS, col = idx % DCOLS;
			const DelaySrc &d = src[s];
			x[q] = 0.0f;
			if (d.line) {
				const uint32_t i = t0 + (col >> 1);
				x[q] = reinterpret_cast<const float *>(g.src)[((size_t)d.row * F + i) * 2 + (col & 1)];
				d.line[GAS_LINE_HEADER + (size_t)((d.p0 + i) & mask) * 2 + (col & 1)] = x[q];
			}
		}
		__syncthreads(); // this tile's ring writes before its tap reads; the previous tile's fb writes before these reads
		// 2. taps and fb[q] whose writer precedes the tile
#pragma unroll
		for (int q = 0; q < DPER; q++) {
			const int idx = q * DNT + tid;
			const int s = idx / DCOLS, col = idx % DCOLS, ear = col & 1;
			const DelaySrc &d = src[s];
			if (d.line) {
				const int i = (int)t0 + (col >> 1);
				const float *ring = d.line + GAS_LINE_HEADER;
				const float r1 = ring[(size_t)((d.p0 + (uint32_t)i - (uint32_t)d.d1) & mask) * 2 + ear];
				const float r2 = ring[(size_t)((d.p0 + (uint32_t)i - (uint32_t)d.d2) & mask) * 2 + ear];
				float o = ((x[q] * d.dry + r1 * d.v1[ear]) + r2 * d.v2[ear]);
				const bool in_tile = i >= d.start && i - d.lc >= d.start && i - d.lc >= (int)t0;
				if (!in_tile) {
					const float *fb = ring + (size_t)(mask + 1) * 2;
					o = o + fb[(size_t)delay_q(i, d.q0, d.lc, d.start) * 2 + ear];
				}
				wo[s * DROW + col] = o;
			}
		}
		__syncthreads();
		// 3. the h chain, one lane of wave 0 per (source, ear)
		if (wave == 0 && line) {
			const int s = lane >> 1, ear = lane & 1;
			float *pw = wo + s * DROW + ear;
			float *pf = fbt + s * DROW + ear;
			if (lc >= KFD) { // no fb value of this tile is read in this tile
				float r[KFD];
#pragma unroll
				for (int k = 0; k < KFD; k++) {
					r[k] = pw[2 * k];
				}
#pragma unroll
				for (int k = 0; k < KFD; k++) {
					h = undenormalize((r[k] * fl) * ic + h * c);
					r[k] = h;
				}
#pragma unroll
				for (int k = 0; k < KFD; k++) {
					pf[2 * k] = r[k];
				}
			} else {
				for (int k = 0; k < KFD; k++) {
					const int i = (int)t0 + k;
					float o = pw[2 * k];
					if (i >= start && i - lc >= start && i - lc >= (int)t0) {
						o = o + pf[2 * (k - lc)];
						pw[2 * k] = o;
					}
					h = undenormalize((o * fl) * ic + h * c);
					pf[2 * k] = h;
				}
			}
		}
		__syncthreads();
		// 4. rows out; fb[q] from the last frame of the tile that writes q
#pragma unroll
		for (int q = 0; q < DPER; q++) {
			const int idx = q * DNT + tid;
			const int s = idx / DCOLS, col = idx % DCOLS, ear = col & 1;
			const DelaySrc &d = src[s];
			if (d.line) {
				const int i = (int)t0 + (col >> 1);
				rows_out[((size_t)(e0 + s) * F + i) * 2 + ear] = wo[s * DROW + col];
				if (!(i >= d.start && i + d.lc < (int)t0 + KFD)) {
					float *fb = d.line + GAS_LINE_HEADER + (size_t)(mask + 1) * 2;
					fb[(size_t)delay_q(i, d.q0, d.lc, d.start) * 2 + ear] = fbt[s * DROW + col];
				}
			} else if (d.out) {
				rows_out[((size_t)(e0 + s) * F + t0 + (col >> 1)) * 2 + ear] = 0.0f;
			}
		}
		// wo / fbt are rewritten after the next tile's first barrier
	}

	if (wave == 0 && line) {
		const int s = lane >> 1, ear = lane & 1;
		uint32_t *hdr = reinterpret_cast<uint32_t *>(line);
		hdr[2 + ear] = __float_as_uint(h);
		if (ear == 0) {
			const DelaySrc &d = src[s];
			const int qe = d.start ? (int)(F - 1) % d.lc : (d.q0 + (int)F) % d.lc;
			hdr[0] = d.p0 + F;
			hdr[1] = (uint32_t)qe;
		}
	}
}

// ---------------------------------------------------------------------------------------------------------------
// GAS_FX_REVERB
// ---------------------------------------------------------------------------------------------------------------
constexpr int RS = 4; // sources per workgroup
constexpr int RR = RS * 2; // mono reverbs per workgroup
constexpr int RNT = 256; // 4 waves; wave 0's lane = (reverb, comb)
constexpr int KFR = 64; // frames per comb tile
constexpr int CTS = KFR + 1; // comb tile row stride: serial lane l reads bank (l + f) % 32
constexpr int MAXF = 512;
constexpr int APB = 8; // allpass elements per thread whose loads are in flight together

// header words of ear e's reverb at 32 e
enum { RH_EPOS = 0, RH_H1, RH_H2, RH_CPOS, RH_DH = RH_CPOS + 8, RH_APOS = RH_DH + 8 };

struct RevSrc { // per mono reverb, LDS
	float *line; // nullptr: no source, or no line entered (never expected; its rows are written as zeros)
	uint32_t row;
	int out; // a group entry: its rows are written
	int pd, e0;
	float pfb, fbk, damp, a1, a2, b1, wet, dry;
	int hp;
	double omd; // 1.0 - damp
	int climit[8], cp0[8], alimit[4], ap0[4];
};

__device__ __forceinline__ int lrintf_dev(float v) {
	return (int)rintf(v);
}

__global__ __launch_bounds__(RNT) void k_fx_reverb(gas_group_args g, gas_dev_state st, gas_line_geo geo, uint32_t F, uint32_t j, float mix_rate, float *__restrict__ rows_out) {
	__shared__ RevSrc rv[RR];
	__shared__ float u[RR * MAXF];
	__shared__ float dsum[RR * MAXF];
	__shared__ float ct[64 * CTS];

	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t e0 = blockIdx.x * RS;
	const size_t stride = st.dyn_stride;
	const double sr = (double)mix_rate;

	// constants; wave 0's lane (r, k) keeps comb k's damping state of reverb r
	float dh = 0.0f;
	if (wave == 0) {
		const int r = lane >> 3, k = lane & 7, s = r >> 1, ear = r & 1;
		const uint32_t e = e0 + s;
		RevSrc &R = rv[r];
		const uint32_t slot = e < g.n ? (g.slots ? g.slots[e] : g.slot_base + e) : 0;
		const int li = e < g.n ? st.line_of[(size_t)j * stride + slot] : -1; // (-1: no line entered; never expected)
		if (li >= 0) {
			const gas_fx_line_settings *P = st.line_settings + slot;
			float *line = st.reverb_pool + (size_t)li * geo.reverb_floats;
			const uint32_t *hdr = reinterpret_cast<const uint32_t *>(line) + 32 * ear;
			const float spread = P->reverb_spread[j];
			const int cut = lrintf_dev((float)((double)(float)geo.xs[ear] * (1.0 - (double)spread)));
			const int cl = (int)geo.comb_size[ear][k] - cut;
			const int cp = (int)hdr[RH_CPOS + k];
			R.climit[k] = cl;
			R.cp0[k] = cp >= cl ? 0 : cp;
			dh = __uint_as_float(hdr[RH_DH + k]);
			if (k < 4) {
				const int al = (int)geo.ap_size[ear][k] - cut;
				const int ap = (int)hdr[RH_APOS + k];
				R.alimit[k] = al;
				R.ap0[k] = ap >= al ? 0 : ap;
			}
			if (k == 0) {
				R.line = line;
				R.out = 1;
				R.row = g.rows ? g.rows[e] : e;
				long pd = lrint((double)P->reverb_predelay_ms[j] / 1000.0 * sr);
				pd = pd < 10 ? 10 : pd;
				pd = pd > (long)geo.echo_size - 1 ? (long)geo.echo_size - 1 : pd;
				R.pd = (int)pd;
				const int ep = (int)hdr[RH_EPOS];
				R.e0 = ep >= (int)geo.echo_size ? 0 : ep;
				R.pfb = P->reverb_predelay_feedback[j];
				double fbk = 0.7 + (double)P->reverb_room_size[j] * 0.28;
				fbk = fbk < 0.7 ? 0.7 : (fbk > 0.98 ? 0.98 : fbk);
				R.fbk = (float)fbk;
				float auxdmp = (float)((double)P->reverb_damping[j] / 2.0 + 0.5);
				auxdmp *= auxdmp;
				R.damp = (float)exp(-TWO_PI * (double)auxdmp * 10000.0 / sr);
				R.omd = 1.0 - (double)R.damp;
				const float hip = P->reverb_hipass[j];
				R.hp = hip > 0.0f;
				const float hpaux = (float)exp(-TWO_PI * (double)hip * 6000.0 / sr);
				R.a1 = (float)((1.0 + (double)hpaux) / 2.0);
				R.a2 = -R.a1;
				R.b1 = hpaux;
				R.wet = P->reverb_wet[j];
				R.dry = P->reverb_dry[j];
			}
		} else if (k == 0) {
			R.line = nullptr;
			R.out = e < g.n;
		}
	}
	__syncthreads();

	const float *X = reinterpret_cast<const float *>(g.src);
	// 1. predelay echo: every read before any write
	constexpr int P1 = RR * MAXF / RNT;
	float in_v[P1];
#pragma unroll
	for (int q = 0; q < P1; q++) {
		const int idx = q * RNT + tid;
		const int r = idx / MAXF, i = idx % MAXF;
		const RevSrc &R = rv[r];
		if (R.line && i < (int)F) {
			const float *echo = R.line + geo.echo_off[r & 1];
			int rd = (R.e0 + i) % (int)geo.echo_size - R.pd;
			rd += rd < 0 ? (int)geo.echo_size : 0;
			const float x = X[((size_t)R.row * F + i) * 2 + (r & 1)];
			in_v[q] = undenormalize(echo[rd] * R.pfb + x);
			u[r * MAXF + i] = in_v[q];
		}
	}
	__syncthreads();
#pragma unroll
	for (int q = 0; q < P1; q++) {
		const int idx = q * RNT + tid;
		const int r = idx / MAXF, i = idx % MAXF;
		const RevSrc &R = rv[r];
		if (R.line && i < (int)F) {
			R.line[geo.echo_off[r & 1] + (R.e0 + i) % (int)geo.echo_size] = in_v[q];
		}
	}
	// 2. high-pass, one lane per reverb (u is in LDS since the barrier above)
	if (wave == 0 && lane < RR && rv[lane].line && rv[lane].hp) {
		const RevSrc &R = rv[lane];
		uint32_t *hdr = reinterpret_cast<uint32_t *>(R.line) + 32 * (lane & 1);
		float h1 = __uint_as_float(hdr[RH_H1]), h2 = __uint_as_float(hdr[RH_H2]);
		const float a1 = R.a1, a2 = R.a2, b1 = R.b1;
		float *pu = u + lane * MAXF;
		for (uint32_t i0 = 0; i0 < F; i0 += 16) {
			float v[16];
#pragma unroll
			for (int k = 0; k < 16; k++) {
				v[k] = pu[i0 + k];
			}
#pragma unroll
			for (int k = 0; k < 16; k++) {
				const float y = (v[k] * a1 + h1 * a2) + h2 * b1;
				h2 = y;
				h1 = v[k];
				v[k] = y;
			}
#pragma unroll
			for (int k = 0; k < 16; k++) {
				pu[i0 + k] = v[k];
			}
		}
		hdr[RH_H1] = __float_as_uint(h1);
		hdr[RH_H2] = __float_as_uint(h2);
	}
	__syncthreads();

	// 3. combs over KFR-frame tiles
	constexpr int P3 = 64 * KFR / RNT;
	for (uint32_t t0 = 0; t0 < F; t0 += KFR) {
#pragma unroll
		for (int q = 0; q < P3; q++) { // thread = (comb lane, frame): reads, undenorm(buf fbk)
			const int idx = q * RNT + tid;
			const int l = idx / KFR, f = idx % KFR, r = l >> 3, k = l & 7;
			const RevSrc &R = rv[r];
			if (R.line) {
				const float *buf = R.line + geo.comb_off[r & 1][k];
				const int pos = (R.cp0[k] + (int)t0 + f) % R.climit[k];
				ct[l * CTS + f] = undenormalize(buf[pos] * R.fbk);
			}
		}
		__syncthreads();
		if (wave == 0 && rv[lane >> 3].line) { // the damping chain, one lane per comb
			const RevSrc &R = rv[lane >> 3];
			const double omd = R.omd;
			const float damp = R.damp;
			float v[KFR];
			float *pc = ct + lane * CTS;
#pragma unroll
			for (int f = 0; f < KFR; f++) {
				v[f] = pc[f];
			}
#pragma unroll
			for (int f = 0; f < KFR; f++) {
				dh = (float)((double)v[f] * omd + (double)(dh * damp));
				v[f] = dh;
			}
#pragma unroll
			for (int f = 0; f < KFR; f++) {
				pc[f] = v[f];
			}
		}
		__syncthreads();
#pragma unroll
		for (int q = 0; q < P3; q++) { // comb writes buf = u + o
			const int idx = q * RNT + tid;
			const int l = idx / KFR, f = idx % KFR, r = l >> 3, k = l & 7;
			const RevSrc &R = rv[r];
			if (R.line) {
				float *buf = R.line + geo.comb_off[r & 1][k];
				const int pos = (R.cp0[k] + (int)t0 + f) % R.climit[k];
				buf[pos] = u[r * MAXF + t0 + f] + ct[l * CTS + f];
			}
		}
		for (int idx = tid; idx < RR * KFR; idx += RNT) { // d = 0 + o_0 + ... + o_7, in comb order
			const int r = idx / KFR, f = idx % KFR;
			if (rv[r].line) {
				float d = 0.0f;
#pragma unroll
				for (int k = 0; k < 8; k++) {
					d += ct[(r * 8 + k) * CTS + f];
				}
				dsum[r * MAXF + t0 + f] = d;
			}
		}
		__syncthreads();
	}

	// 4. allpasses in series, each in rounds of `limit` frames (a round's frames touch distinct positions)
	for (int k = 0; k < 4; k++) {
		const int rounds = ((int)F + (int)geo.ap_base[k] - 1) / (int)geo.ap_base[k];
		const int cap = (int)geo.ap_size[1][k]; // >= every limit of allpass k
		for (int rho = 0; rho < rounds; rho++) {
			for (int base = 0; base < RR * cap; base += RNT * APB) {
				// APB loads in flight before any store: a round's positions are distinct, so none of them aliases
				float *bp[APB];
				int pos[APB], di[APB];
				float aux[APB];
#pragma unroll
				for (int q = 0; q < APB; q++) {
					const int idx = base + q * RNT + tid;
					const int r = idx / cap, f = idx % cap;
					bp[q] = nullptr;
					pos[q] = di[q] = 0;
					aux[q] = 0.0f;
					if (idx < RR * cap) {
						const RevSrc &R = rv[r];
						const int L = R.alimit[k];
						const int i = rho * L + f;
						if (R.line && f < L && i < (int)F) {
							bp[q] = R.line + geo.ap_off[r & 1][k];
							pos[q] = (R.ap0[k] + i) % L;
							di[q] = r * MAXF + i;
							aux[q] = bp[q][pos[q]];
						}
					}
				}
#pragma unroll
				for (int q = 0; q < APB; q++) {
					if (bp[q]) {
						const float nb = undenormalize(0.7f * aux[q] + dsum[di[q]]);
						bp[q][pos[q]] = nb;
						dsum[di[q]] = aux[q] - 0.7f * nb;
					}
				}
			}
			__syncthreads();
		}
	}

	// 5. rows out
	for (int idx = tid; idx < RS * (int)F * 2; idx += RNT) {
		const int s = idx / ((int)F * 2), col = idx % ((int)F * 2), i = col >> 1, ear = col & 1, r = s * 2 + ear;
		const RevSrc &R = rv[r];
		if (R.line) {
			const float x = X[((size_t)R.row * F + i) * 2 + ear];
			rows_out[((size_t)(e0 + s) * F) * 2 + col] = ((dsum[r * MAXF + i] * R.wet) * 0.6f) + x * R.dry;
		} else if (R.out) {
			rows_out[((size_t)(e0 + s) * F) * 2 + col] = 0.0f;
		}
	}

	// positions after the block (not wrapped: the next use checks), comb damping state
	if (wave == 0 && rv[lane >> 3].line) {
		const int r = lane >> 3, k = lane & 7;
		const RevSrc &R = rv[r];
		uint32_t *hdr = reinterpret_cast<uint32_t *>(R.line) + 32 * (r & 1);
		hdr[RH_CPOS + k] = (uint32_t)((R.cp0[k] + (int)F - 1) % R.climit[k] + 1);
		hdr[RH_DH + k] = __float_as_uint(dh);
		if (k < 4) {
			hdr[RH_APOS + k] = (uint32_t)((R.ap0[k] + (int)F - 1) % R.alimit[k] + 1);
		}
		if (k == 0) {
			hdr[RH_EPOS] = (uint32_t)((R.e0 + (int)F - 1) % (int)geo.echo_size + 1);
		}
	}
}

} // namespace

hipError_t gas_launch_fx_line(hipStream_t stream, int kind, const gas_group_args &g, const gas_dev_state &st, const gas_line_geo &geo, uint32_t frames, uint32_t chain_pos, float mix_rate, gas_audio_frame *rows_out) {
	if (g.n == 0) {
		return hipSuccess;
	}
	if (frames % KFR != 0 || frames > MAXF || chain_pos >= GAS_MAX_EFFECTS) {
		return hipErrorInvalidValue;
	}
	float *out = reinterpret_cast<float *>(rows_out);
	if (kind == GAS_FX_DELAY && st.delay_pool) {
		hipLaunchKernelGGL(k_fx_delay, dim3((g.n + DS - 1) / DS), dim3(DNT), 0, stream, g, st, geo, frames, chain_pos, mix_rate, out);
	} else if (kind == GAS_FX_REVERB && st.reverb_pool) {
		hipLaunchKernelGGL(k_fx_reverb, dim3((g.n + RS - 1) / RS), dim3(RNT), 0, stream, g, st, geo, frames, chain_pos, mix_rate, out);
	} else {
		return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
