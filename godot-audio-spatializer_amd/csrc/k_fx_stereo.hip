// k_fx_stereo.hip -- the engine's panner, stereo enhance and limiter as stages of a staged effect chain (rows in ->
// dense rows out).  Settings from gas_fx_stereo_settings by chain position, read once per block (no
// ramp).  Panner and limiter hold no state; a stereo enhance holds one mono ring from the pool of
// gas_ctx_reserve_fx_stereo (addressed through st.stereo_of).  The semantics are a recollection of the engine's
// audio_effect_panner.cpp, audio_effect_stereo_enhance.cpp and audio_effect_limiter.cpp, not pinned against its source
// (like SURVEY Appendix B).  Block constants are computed in f64 and rounded to f32; the limiter's per-sample log and
// exp are evaluated in f64 and rounded, so no device logf / expf approximation enters the result.  sr is the mix rate
// (f64), db2lin(x) = exp(x 0.11512925464970228), lin2db(x) = log(x) 8.685889638065035.
//
//   GAS_FX_PANNER  lvol = (float)clamp(1 - pan, 0, 1), rvol = (float)clamp(1 + pan, 0, 1), cl = (float)(1 - lvol),
//       cr = (float)(1 - rvol); per frame (L, R): L' = L lvol + R cr, R' = R rvol + L cl.
//   GAS_FX_STEREO_ENHANCE  state: a mono ring of R frames and pos (u32).  delay = (unsigned)(ms / 1000 sr),
//       p = pan_pullout; per frame: c = (L + R) / 2, l = c + (L - c) p, r = c + (R - c) p;
//       surround > 0: ring[pos] = (l + r) / 2, o = ring[pos - delay] surround, l = l + o, r = r - o;
//       else: ring[pos] = r, r = ring[pos - delay];  pos++.  The write comes before the read: delay 0 reads this
//       frame's value.  The ring keeps whatever mode wrote it.
//   GAS_FX_LIMITER  ceiling = db2lin(ceil_db), makeup = db2lin(ceil_db - thr_db), sc = -soft_clip_db, scv = db2lin(sc),
//       scmult = |(ceil_db - sc) / ((ceil_db + 25) - sc)|; per ear: s = x makeup, a = |s|, sign = s < 0 ? -1 : 1;
//       a > scv: s = sign (scv + db2lin((lin2db(a) - ceil_db) scmult));  y = min(ceiling, |s|) (s < 0 ? -1 : 1).
//
// Mapping: no recurrence over frames, so no serial lane.  SS sources per workgroup; the first SS threads compute the
// sources' block constants into LDS; then a thread per two frames, both ears of both frames in one 16-byte access,
// coalesced over the row.  The stereo enhance computes every (l, r) of the block in place into LDS first -- the value
// the ring would receive at a frame follows from that frame's (l, r) alone -- then takes a delayed value from LDS where
// its frame lies in this block and from the ring where it is older, and writes the whole block into the ring after
// every read of the launch (a barrier apart; a source's ring is touched by its own workgroup only).  That order needs
// ring frames >= block frames (no two frames of a block on one ring entry) and > delay (gas_ctx_reserve_fx_stereo).
// No FMA contraction: products and sums round like the engine's separate f32 operations.
#include <cmath>

#include "gas_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t MAXF = 512;
constexpr int SS = 2; // sources per workgroup
constexpr int SNT = 256; // 4 waves
constexpr double DB2LIN = 0.11512925464970228, LIN2DB = 8.685889638065035;

struct StereoSrc { // per source, LDS
	int out; // 1: process; 0: an entry whose state is missing (never expected; zeros); -1: no entry
	uint32_t row;
	float k[5]; // panner: lvol, rvol, cl, cr; enhance: pullout, surround; limiter: ceiling, makeup, scv, scmult, ceil_db
	float *ring; // enhance
	uint32_t pos, delay;
};

__device__ __forceinline__ float clamp01f(double v) {
	return (float)(v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v));
}

__device__ __forceinline__ float limit(float x, const float *k) {
	float s = x * k[1];
	const float a = fabsf(s);
	if (a > k[2]) {
		const float sign = s < 0.0f ? -1.0f : 1.0f;
		const float over = (float)(log((double)a) * LIN2DB) - k[4];
		s = sign * (k[2] + (float)exp((double)(over * k[3]) * DB2LIN));
	}
	return fminf(k[0], fabsf(s)) * (s < 0.0f ? -1.0f : 1.0f);
}

template <int KIND>
__global__ __launch_bounds__(SNT) void k_fx_stereo(gas_group_args g, gas_dev_state st, uint32_t F, uint32_t j, float mix_rate, float *__restrict__ rows_out) {
	constexpr bool ENH = KIND == GAS_FX_STEREO_ENHANCE;
	__shared__ StereoSrc src[SS];
	__shared__ float4 lr[ENH ? SS * MAXF / 2 : 1]; // enhance: (l, r) of every frame of the block, two frames per entry

	const int tid = threadIdx.x;
	const uint32_t e0 = blockIdx.x * SS;
	const uint32_t H = F / 2; // 16-byte pieces of a row
	const uint32_t mask = st.enhance_mask;

	if (tid < SS) {
		const uint32_t e = e0 + tid;
		StereoSrc d;
		d.out = e < g.n ? 1 : -1;
		d.ring = nullptr;
		d.pos = d.delay = 0;
		d.row = 0;
		for (int q = 0; q < 5; q++) {
			d.k[q] = 0.0f;
		}
		if (e < g.n) {
			const uint32_t slot = g.slots ? g.slots[e] : g.slot_base + e;
			const gas_fx_stereo_settings *P = st.stereo_settings + slot;
			d.row = g.rows ? g.rows[e] : e;
			if (KIND == GAS_FX_PANNER) {
				const double pan = (double)P->panner_pan[j];
				d.k[0] = clamp01f(1.0 - pan);
				d.k[1] = clamp01f(1.0 + pan);
				d.k[2] = (float)(1.0 - (double)d.k[0]);
				d.k[3] = (float)(1.0 - (double)d.k[1]);
			} else if (ENH) {
				const int ri = st.stereo_of[(size_t)j * st.dyn_stride + slot];
				if (ri >= 0 && st.enhance_pool) {
					d.ring = st.enhance_pool + (size_t)ri * (GAS_ENHANCE_HEADER + (size_t)mask + 1);
					d.pos = reinterpret_cast<const uint32_t *>(d.ring)[0];
					d.delay = (unsigned)((double)P->enhance_time_pullout_ms[j] / 1000.0 * (double)mix_rate);
					d.delay = d.delay > mask ? mask : d.delay; // (never: ring frames > 0.05 sr)
					d.k[0] = P->enhance_pan_pullout[j];
					d.k[1] = P->enhance_surround[j];
				} else {
					d.out = 0;
				}
			} else {
				const double ceil_db = (double)P->limiter_ceiling_db[j], sc = -(double)P->limiter_soft_clip_db[j];
				d.k[0] = (float)exp(ceil_db * DB2LIN);
				d.k[1] = (float)exp((ceil_db - (double)P->limiter_threshold_db[j]) * DB2LIN);
				d.k[2] = (float)exp(sc * DB2LIN);
				d.k[3] = (float)fabs((ceil_db - sc) / ((ceil_db + 25.0) - sc));
				d.k[4] = P->limiter_ceiling_db[j];
			}
		}
		src[tid] = d;
	}
	__syncthreads();

	const float4 *in = reinterpret_cast<const float4 *>(g.src);
	float4 *outp = reinterpret_cast<float4 *>(rows_out);

	if (!ENH) {
		for (uint32_t idx = tid; idx < SS * H; idx += SNT) {
			const uint32_t s = idx / H, p = idx % H;
			const StereoSrc &c = src[s];
			if (c.out < 0) {
				continue;
			}
			const float4 x = in[(size_t)c.row * H + p];
			float4 y;
			if (KIND == GAS_FX_PANNER) {
				y.x = x.x * c.k[0] + x.y * c.k[3];
				y.y = x.y * c.k[1] + x.x * c.k[2];
				y.z = x.z * c.k[0] + x.w * c.k[3];
				y.w = x.w * c.k[1] + x.z * c.k[2];
			} else {
				y.x = limit(x.x, c.k);
				y.y = limit(x.y, c.k);
				y.z = limit(x.z, c.k);
				y.w = limit(x.w, c.k);
			}
			outp[(size_t)(e0 + s) * H + p] = y;
		}
		return;
	}

	// 1. (l, r) of every frame of the block
	for (uint32_t idx = tid; idx < SS * H; idx += SNT) {
		const uint32_t s = idx / H, p = idx % H;
		const StereoSrc &c = src[s];
		if (c.out <= 0) {
			continue;
		}
		const float4 x = in[(size_t)c.row * H + p];
		const float pull = c.k[0];
		const float c0 = (x.x + x.y) * 0.5f, c1 = (x.z + x.w) * 0.5f;
		lr[s * (MAXF / 2) + p] = make_float4(c0 + (x.x - c0) * pull, c0 + (x.y - c0) * pull, c1 + (x.z - c1) * pull, c1 + (x.w - c1) * pull);
	}
	__syncthreads();
	// 2. the delayed values, from the block where they lie in it and from the ring where they are older; rows out
	const float2 *lrf = reinterpret_cast<const float2 *>(lr); // one frame's (l, r) in one 8-byte LDS access
	for (uint32_t idx = tid; idx < SS * H; idx += SNT) {
		const uint32_t s = idx / H, p = idx % H;
		const StereoSrc &c = src[s];
		if (c.out < 0) {
			continue;
		}
		float4 y = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (c.out > 0) {
			y = lr[s * (MAXF / 2) + p];
			const bool sur = c.k[1] > 0.0f;
			float d[2];
#pragma unroll
			for (uint32_t q = 0; q < 2; q++) {
				const uint32_t i = 2 * p + q;
				if (i >= c.delay) {
					const float2 v = lrf[s * MAXF + (i - c.delay)];
					d[q] = sur ? (v.x + v.y) * 0.5f : v.y;
				} else {
					d[q] = c.ring[GAS_ENHANCE_HEADER + ((c.pos + i - c.delay) & mask)];
				}
			}
			if (sur) {
				const float o0 = d[0] * c.k[1], o1 = d[1] * c.k[1];
				y.x = y.x + o0;
				y.y = y.y - o0;
				y.z = y.z + o1;
				y.w = y.w - o1;
			} else {
				y.y = d[0];
				y.w = d[1];
			}
		}
		outp[(size_t)(e0 + s) * H + p] = y;
	}
	__syncthreads();
	// 3. the block into the ring, after every read of it; then the state
	for (uint32_t idx = tid; idx < SS * F; idx += SNT) {
		const uint32_t s = idx / F, i = idx % F;
		const StereoSrc &c = src[s];
		if (c.out > 0) {
			const float2 v = lrf[s * MAXF + i];
			c.ring[GAS_ENHANCE_HEADER + ((c.pos + i) & mask)] = c.k[1] > 0.0f ? (v.x + v.y) * 0.5f : v.y;
		}
	}
	if (tid < SS && src[tid].out > 0) {
		reinterpret_cast<uint32_t *>(src[tid].ring)[0] = src[tid].pos + F;
	}
}

} // namespace

hipError_t gas_launch_fx_stereo(hipStream_t stream, int kind, const gas_group_args &g, const gas_dev_state &st, uint32_t frames, uint32_t chain_pos, float mix_rate, gas_audio_frame *rows_out) {
	if (g.n == 0) {
		return hipSuccess;
	}
	if (frames % 2 != 0 || frames == 0 || frames > MAXF || chain_pos >= GAS_MAX_EFFECTS || !st.stereo_settings || !st.stereo_of) {
		return hipErrorInvalidValue;
	}
	float *out = reinterpret_cast<float *>(rows_out);
	const dim3 grid((g.n + SS - 1) / SS), block(SNT);
	if (kind == GAS_FX_PANNER) {
		hipLaunchKernelGGL(k_fx_stereo<GAS_FX_PANNER>, grid, block, 0, stream, g, st, frames, chain_pos, mix_rate, out);
	} else if (kind == GAS_FX_LIMITER) {
		hipLaunchKernelGGL(k_fx_stereo<GAS_FX_LIMITER>, grid, block, 0, stream, g, st, frames, chain_pos, mix_rate, out);
	} else if (kind == GAS_FX_STEREO_ENHANCE && st.enhance_pool && st.enhance_mask + 1 >= frames) {
		hipLaunchKernelGGL(k_fx_stereo<GAS_FX_STEREO_ENHANCE>, grid, block, 0, stream, g, st, frames, chain_pos, mix_rate, out);
	} else {
		return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
