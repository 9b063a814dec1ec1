// k_fx_dyn.hip -- the engine's nonlinear and dynamics effects as stages of a staged effect chain (rows in -> dense rows
// out), settings from gas_fx_dyn_settings by chain position, read once per block (no ramps):
//
//   GAS_FX_DISTORTION  [ENGINE] AudioEffectDistortionInstance::process.  Ears independent; state h[ear] per slot and
//     chain position.  Block constants (f64, rounded to f32):
//       c = exp(-2 pi keep_hf_hz / mix_rate), ic = 1 - c, pre = db2lin(pre_gain_db), post = db2lin(post_gain_db), d = drive
//       atan_mult = 10^(3 d^2) - 1 + 0.001, atan_div = 1 / (atan(atan_mult) (1 + 8 d)), lofi_mult = 2^(2 + 14 (1 - d))
//     per sample x:
//       lo = undenorm(x ic + c h)   (|v| < 2^-111 -> 0),   h = lo,   hf = x - lo,   a = lo pre
//       CLIP       a = sign(a) |a|^(1.0001 - d), clamped to [-1, 1]
//       ATAN       a = atanf(a atan_mult) atan_div
//       LOFI       a = floorf(a lofi_mult + 0.5) / lofi_mult
//       OVERDRIVE  in f64: x' = a 0.686306, z = 1 + exp(-0.75 sqrt|x'|), a = (e^x' - e^(-x' z)) / (e^x' + e^-x')
//       WAVESHAPE  k = 2 d / (1.00001 - d), in f64: a = (1 + k) a / (1 + k |a|)
//       y = a post + hf
//   GAS_FX_COMPRESSOR  [ENGINE] AudioEffectCompressorInstance::process.  Stereo-linked; the only state that reaches the
//     output is rundb per slot and chain position (the engine's averatio / runratio / runmax / maxover / gr_meter do
//     not: its ratio is always `ratio`).  Block constants (f64, rounded to f32):
//       thr = db2lin(threshold_db), at = exp(-1 / (attack_us 1e-6 sr)), rel = exp(-1 / (release_ms 1e-3 sr)), mk = db2lin(gain_db)
//     per frame i, with s = compressor_sidechain[j] and x the playback's own frame:
//       d = s == 0 ? x[i] : key[s - 1][i]        (the engine's sidechain bus: a key block of the context, gas_sidechain_set)
//       over = max(0, 2.08136898 lin2db(max(|d.l|, |d.r|) / thr))    (silence: lin2db = -inf -> 0)
//       rundb = over + (over > rundb ? at : rel) (rundb - over)
//       g = db2lin(-rundb (ratio - 1) / ratio),   y = ((x g) mk) mix + x (1 - mix) per ear
//     The detector alone reads the key: the gain always lands on x, and rundb is the one state whatever s is (changing s
//     between blocks keeps it).  The peak is divided by the source's own thr and goes through the one logf either way, so
//     a key equal to the source's row gives the keyless result to the bit.
//   db2lin(x) = exp(x 0.11512925464970228), lin2db(x) = log(x) 8.685889638065035.
//
// Geometry (wave64, NW = 8 waves per workgroup): S sources per workgroup -- 32 for the distortion (wave 0's lane =
// source, ear), 64 for the compressor (wave 0's lane = source).  The rows are staged through LDS in [S x KF frames] tiles
// with coalesced 16-byte loads by all waves (the next tile's loads in flight during the current one, as k_biquad_mix
// does), and every tile runs in three phases:
//   1. across all waves: what does not depend on the recurrence -- the distortion's input products x ic, the
//      compressor's detector (peak of the source's frame or of its key's, logf, scale, clamp);
//   2. wave 0, one serial lane per recurrence, in the engine's order (not scanned: keep_hf_hz puts c next to 1, where scans leave
//      the parity band) -- per step only add / mul / select for the distortion, compare / select / sub / mul / add for
//      the compressor;
//   3. across all waves again: the waveshaper and output of the distortion (one source per wave and step of the loop, so
//      the mode is wave-uniform), the compressor's gain (expf) and output.
// Sidechain keys: the key frames of a tile are the same for every source of the workgroup, so they are staged once per
// tile as kpk[key][frame] = max(|l|, |r|) (GAS_MAX_SIDECHAINS x KF floats, 1 KiB) by the first 256 threads, each with one
// 8-byte load a tile ahead like the rows, instead of a global read per (source, frame).  Whether any source of the
// workgroup names a key is a ballot every wave takes over the same 64 settings words: workgroup-uniform, and a launch
// without keys does nothing of this beyond that branch.
// MEASURED (profiles/r04_fx_dyn_notes.md): with one wave per workgroup the per-sample transcendentals of phases 1 and 3,
// not the recurrence, bounded the stage (275 us at 256 and at 8192 sources); eight waves share them.
// No FMA contraction: the recurrences and products round like the engine's separate f32 operations.
#include <cmath>
#include <type_traits>

#include "gas_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int KF = 32; // frames per staged tile
constexpr int COLS = KF * 2; // floats of one source per tile (interleaved ears)
constexpr int ROW = COLS + 2; // LDS row stride in floats: serial lane (s, ear) reads bank (2 s + ear + 2 k) % 32, distinct over a half-wave
constexpr int PARTS = COLS / 4; // 16-byte pieces of one source's tile row
constexpr int OW = KF + 1; // compressor detector row stride: serial lane s reads bank (s + k) % 32
constexpr int NW = 8; // waves per workgroup
constexpr int NT = 64 * NW;
// compressor key peaks kpk[key][frame] (behind the detector rows in `work`), row stride KF: phase 1's thread = (source, frame) puts one source on each
// 32-lane half of a wave, so a half reads ONE row at banks f % 32, all distinct (two halves never conflict; sources on
// the same key read the same addresses); the staging thread (key, frame) = (tid / KF, tid % KF) writes the same way
constexpr int KEYS = GAS_MAX_SIDECHAINS;
static_assert(KEYS * KF <= NT, "one staging thread per (key, frame) of a tile");

template <int KIND>
struct Geo {
	static constexpr int S = KIND == GAS_FX_DISTORTION ? 32 : 64;
	static constexpr int LOADS = S * PARTS / NT; // staging loads per thread per tile
	static constexpr int WORK = KIND == GAS_FX_DISTORTION ? S * ROW : S * OW + GAS_MAX_SIDECHAINS * KF; // the compressor's: detector rows, then the key peaks
};

// constants per source in LDS (phases 1 and 3)
enum { DC_IC = 0, DC_PRE, DC_POST, DC_P1, DC_P2, DC_N };
enum { CC_THR = 0, CC_RM1, CC_RATIO, CC_MK, CC_MIX, CC_OMIX, CC_N };

__device__ __forceinline__ float undenormalize(float v) { // [ENGINE] undenormalize: biased exponent < 16 -> 0
	return (__float_as_uint(v) & 0x7f800000u) < 0x08000000u ? 0.0f : v;
}

__device__ __forceinline__ float db2lin_block(float db) {
	return (float)exp((double)db * 0.11512925464970228);
}

__device__ __forceinline__ float shape(int mode, float a, float p1, float p2) {
	switch (mode) {
		case GAS_DISTORTION_CLIP: { // p1 = 1.0001 - d
			const float a_sign = a < 0.0f ? -1.0f : 1.0f;
			a = powf(fabsf(a), p1) * a_sign;
			a = a > 1.0f ? 1.0f : (a < -1.0f ? -1.0f : a);
		} break;
		case GAS_DISTORTION_ATAN: // p1 = atan_mult, p2 = atan_div
			a = atanf(a * p1) * p2;
			break;
		case GAS_DISTORTION_LOFI: // p1 = lofi_mult
			a = floorf(a * p1 + 0.5f) / p1;
			break;
		case GAS_DISTORTION_OVERDRIVE: {
			const double x = (double)a * 0.686306;
			const double z = 1.0 + exp(sqrt(fabs(x)) * -0.75);
			a = (float)((exp(x) - exp(-x * z)) / (exp(x) + exp(-x)));
		} break;
		default: { // WAVESHAPE, p1 = k
			const double k = (double)p1;
			a = (float)((1.0 + k) * (double)a / (1.0 + k * fabs((double)a)));
		} break;
	}
	return a;
}

template <int KIND>
__global__ __launch_bounds__(NT) void k_fx_dyn(gas_group_args g, gas_dev_state st, uint32_t F, uint32_t j, float mix_rate, float *__restrict__ rows_out) {
	constexpr int S = Geo<KIND>::S, LOADS = Geo<KIND>::LOADS;
	constexpr bool DIST = KIND == GAS_FX_DISTORTION;
	__shared__ float tile[2][S * ROW];
	__shared__ float work[Geo<KIND>::WORK];
	__shared__ float cst[DIST ? DC_N : CC_N][S];
	__shared__ int mode_s[S]; // the distortion's mode; the compressor's sidechain (0: none, k: key k - 1)

	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t e0 = blockIdx.x * S;
	const int me = DIST ? lane >> 1 : lane; // this lane's source within the workgroup
	const int ear = DIST ? lane & 1 : 0;
	const uint32_t e = e0 + me;
	const bool valid = e < g.n;
	const uint32_t ec = valid ? e : g.n - 1;
	const uint32_t slot = g.slots ? g.slots[ec] : g.slot_base + ec;
	const gas_fx_dyn_settings *P = st.dyn + slot;
	const size_t stride = st.dyn_stride;
	// the compressor's sidechain word of this lane's source, in every wave: issued here, looked at behind the staging loads
	[[maybe_unused]] uint32_t side = 0;
	if constexpr (!DIST) {
		side = valid ? P->compressor_sidechain[j] : 0u;
	}

	// block constants and state of this lane's recurrence (wave 0)
	float c = 0.0f, at = 0.0f, rel = 0.0f, h = 0.0f;
	if (wave != 0) {
	} else if constexpr (DIST) {
		const float d = P->distortion_drive[j];
		const int mode = P->distortion_mode[j];
		c = (float)exp(-2.0 * M_PI * (double)P->distortion_keep_hf_hz[j] / (double)mix_rate);
		float p1 = 0.0f, p2 = 0.0f;
		if (mode == GAS_DISTORTION_CLIP) {
			p1 = (float)(1.0001 - (double)d);
		} else if (mode == GAS_DISTORTION_ATAN) {
			p1 = (float)(pow(10.0, (double)(d * d) * 3.0) - 1.0 + 0.001);
			p2 = (float)(1.0 / ((double)(float)atan((double)p1) * (1.0 + (double)(d * 8.0f))));
		} else if (mode == GAS_DISTORTION_LOFI) {
			p1 = (float)pow(2.0, 2.0 + (1.0 - (double)d) * 14.0);
		} else if (mode == GAS_DISTORTION_WAVESHAPE) {
			p1 = (float)((double)(2.0f * d) / (1.00001 - (double)d));
		}
		if (ear == 0) {
			cst[DC_IC][me] = 1.0f - c;
			cst[DC_PRE][me] = db2lin_block(P->distortion_pre_gain_db[j]);
			cst[DC_POST][me] = db2lin_block(P->distortion_post_gain_db[j]);
			cst[DC_P1][me] = p1;
			cst[DC_P2][me] = p2;
			mode_s[me] = mode;
		}
		h = st.dist_h[((size_t)j * 2 + ear) * stride + slot];
	} else {
		const double sr = (double)mix_rate;
		const float ratio = P->compressor_ratio[j];
		const float mix = P->compressor_mix[j];
		at = (float)exp(-1.0 / ((double)P->compressor_attack_us[j] * 1e-6 * sr));
		rel = (float)exp(-1.0 / ((double)P->compressor_release_ms[j] * 1e-3 * sr));
		cst[CC_THR][me] = db2lin_block(P->compressor_threshold_db[j]);
		cst[CC_RM1][me] = ratio - 1.0f;
		cst[CC_RATIO][me] = ratio;
		cst[CC_MK][me] = db2lin_block(P->compressor_gain_db[j]);
		cst[CC_MIX][me] = mix;
		cst[CC_OMIX][me] = 1.0f - mix;
		h = st.comp_rundb[(size_t)j * stride + slot]; // rundb
	}

	// staging: load q of this thread covers source idx / PARTS, 16-byte piece idx % PARTS of the tile (idx = q * NT + tid)
	const float *ld[LOADS];
	float *sto[LOADS];
#pragma unroll
	for (int q = 0; q < LOADS; q++) {
		const int idx = q * NT + tid;
		const uint32_t le = e0 + idx / PARTS;
		const uint32_t lc = le < g.n ? le : g.n - 1;
		const uint32_t lrow = g.rows ? g.rows[lc] : lc;
		ld[q] = reinterpret_cast<const float *>(g.src) + (size_t)lrow * F * 2 + (idx % PARTS) * 4;
		sto[q] = le < g.n ? rows_out + (size_t)le * F * 2 + (idx % PARTS) * 4 : nullptr;
	}
	float4 pre[LOADS];
#pragma unroll
	for (int q = 0; q < LOADS; q++) {
		pre[q] = *reinterpret_cast<const float4 *>(ld[q]);
	}
	// sidechain keys: the compressor instantiation only
	[[maybe_unused]] bool any_key = false, key_thread = false;
	[[maybe_unused]] uint32_t koff = 0;
	[[maybe_unused]] float2 kpre = make_float2(0.0f, 0.0f);
	[[maybe_unused]] float *const kpk = work + S * OW;
	[[maybe_unused]] const float2 *const keys = reinterpret_cast<const float2 *>(st.sidechain);
	if constexpr (!DIST) {
		// lane = source in every wave: all eight ballots see the same 64 words.  Behind the staging loads, so that no
		// wave holds those back for the settings word
		side = side > (uint32_t)KEYS ? 0u : side; // (a publish never lets such a value through)
		any_key = __ballot(side != 0) != 0;
		if (wave == 0) {
			mode_s[me] = (int)side;
		}
		// key staging: thread (key, frame) of the tile, its frame loaded a tile ahead
		key_thread = any_key && tid < KEYS * KF;
		koff = (uint32_t)(tid / KF) * F + tid % KF; // < GAS_MAX_SIDECHAINS * F for a key thread
		if (key_thread) {
			kpre = keys[koff];
		}
	}

	const uint32_t n_tiles = F / KF;
	for (uint32_t tl = 0; tl < n_tiles; tl++) {
		float *tb = tile[tl & 1];
#pragma unroll
		for (int q = 0; q < LOADS; q++) { // rows are 264 B apart: two 8-byte stores
			const int idx = q * NT + tid;
			float *d = tb + (idx / PARTS) * ROW + (idx % PARTS) * 4;
			*reinterpret_cast<float2 *>(d) = make_float2(pre[q].x, pre[q].y);
			*reinterpret_cast<float2 *>(d + 2) = make_float2(pre[q].z, pre[q].w);
		}
		if constexpr (!DIST) {
			if (key_thread) { // last read in phase 1 of the previous tile, three barriers ago
				const float l = fabsf(kpre.x), r = fabsf(kpre.y);
				kpk[tid] = l > r ? l : r; // [tid / KF][tid % KF]
			}
		}
		if (tl + 1 < n_tiles) {
#pragma unroll
			for (int q = 0; q < LOADS; q++) {
				pre[q] = *reinterpret_cast<const float4 *>(ld[q] + (size_t)(tl + 1) * COLS);
			}
			if constexpr (!DIST) {
				if (key_thread) {
					kpre = keys[koff + (tl + 1) * KF];
				}
			}
		}
		__syncthreads();

		// 1. across all waves
		if constexpr (DIST) {
			for (int s = wave; s < S; s += NW) { // lane = column (frame, ear) of source s
				work[s * ROW + lane] = tb[s * ROW + lane] * cst[DC_IC][s];
			}
		} else {
			auto detect = [&](auto keyed) { // the keyless loop is the one loop there was: the choice is made outside it
				for (int it = 0; it < S * KF / NT; it++) { // thread = (source, frame)
					const int idx = it * NT + tid;
					const int s = idx / KF, f = idx % KF;
					const float l = fabsf(tb[s * ROW + 2 * f]), r = fabsf(tb[s * ROW + 2 * f + 1]);
					float peak = l > r ? l : r;
					if constexpr (decltype(keyed)::value) {
						const int k = mode_s[s];
						const float key_peak = kpk[((k != 0 ? k : 1) - 1) * KF + f];
						peak = k != 0 ? key_peak : peak;
					}
					float over = 2.08136898f * (logf(peak / cst[CC_THR][s]) * 8.685889638065035f);
					over = over < 0.0f ? 0.0f : over; // (-inf for silence)
					work[s * OW + f] = over;
				}
			};
			if (any_key) {
				detect(std::true_type());
			} else {
				detect(std::false_type());
			}
		}
		__syncthreads();

		// 2. the recurrence, one lane of wave 0 each, in the engine's order
		if (wave == 0) {
			float *p = DIST ? work + me * ROW + ear : work + me * OW;
			constexpr int STEP = DIST ? 2 : 1;
			float r[KF];
#pragma unroll
			for (int k = 0; k < KF; k++) {
				r[k] = p[STEP * k];
			}
#pragma unroll
			for (int k = 0; k < KF; k++) {
				if constexpr (DIST) {
					const float lo = undenormalize(r[k] + c * h); // x ic + c h
					h = lo;
					r[k] = lo;
				} else {
					const float over = r[k];
					h = over + (over > h ? at : rel) * (h - over);
					r[k] = h;
				}
			}
#pragma unroll
			for (int k = 0; k < KF; k++) {
				p[STEP * k] = r[k];
			}
		}
		__syncthreads();

		// 3. across all waves: shape / gain and output, one source per wave and step (lane = column)
		for (int s = wave; s < S; s += NW) {
			const int a_ = s * ROW + lane;
			const float x = tb[a_];
			if constexpr (DIST) {
				const float lo = work[a_];
				const float a = shape(mode_s[s], lo * cst[DC_PRE][s], cst[DC_P1][s], cst[DC_P2][s]);
				tb[a_] = a * cst[DC_POST][s] + (x - lo);
			} else {
				const float rundb = work[s * OW + (lane >> 1)];
				const float gr = (-rundb * cst[CC_RM1][s]) / cst[CC_RATIO][s];
				const float gv = expf(gr * 0.11512925464970228f);
				tb[a_] = ((x * gv) * cst[CC_MK][s]) * cst[CC_MIX][s] + x * cst[CC_OMIX][s];
			}
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
		// the next tile fills the other buffer; this one is rewritten after the next tile's barrier
	}

	if (wave == 0 && valid) {
		if constexpr (DIST) {
			st.dist_h[((size_t)j * 2 + ear) * stride + slot] = h;
		} else {
			st.comp_rundb[(size_t)j * stride + slot] = h;
		}
	}
}

} // namespace

hipError_t gas_launch_fx_dyn(hipStream_t stream, int kind, const gas_group_args &g, const gas_dev_state &st, uint32_t frames, uint32_t chain_pos, float mix_rate, gas_audio_frame *rows_out) {
	if (g.n == 0) {
		return hipSuccess;
	}
	if (frames % KF != 0 || chain_pos >= GAS_MAX_EFFECTS) {
		return hipErrorInvalidValue;
	}
	float *out = reinterpret_cast<float *>(rows_out);
	if (kind == GAS_FX_DISTORTION) {
		hipLaunchKernelGGL(k_fx_dyn<GAS_FX_DISTORTION>, dim3((g.n + Geo<GAS_FX_DISTORTION>::S - 1) / Geo<GAS_FX_DISTORTION>::S), dim3(NT), 0, stream, g, st, frames, chain_pos, mix_rate, out);
	} else if (kind == GAS_FX_COMPRESSOR) {
		hipLaunchKernelGGL(k_fx_dyn<GAS_FX_COMPRESSOR>, dim3((g.n + Geo<GAS_FX_COMPRESSOR>::S - 1) / Geo<GAS_FX_COMPRESSOR>::S), dim3(NT), 0, stream, g, st, frames, chain_pos, mix_rate, out);
	} else {
		return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
