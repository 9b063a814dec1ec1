// k_fx_mod.hip -- the engine's chorus and phaser as stages of a staged effect chain (rows in -> dense rows out,
// DESIGN.md 3.5g).  Settings from gas_fx_mod_settings by chain position, read once per block (no ramp); state in one
// chorus line or phaser bank per effect instance, from the pools of gas_ctx_reserve_fx_mod (addressed through
// st.mod_of).  The semantics are a recollection of the engine's audio_effect_chorus.cpp and audio_effect_phaser.cpp,
// not pinned against its source (like SURVEY Appendix B).  Block constants are computed in f64 and rounded to f32;
// every sine is (float)sin((double)arg), so no device sinf approximation enters the result.  TAU = 2 pi (f64), sr the
// mix rate (f64), db2lin k_fx_dyn.hip's.
//
//   GAS_FX_CHORUS  state: a stereo ring of R frames, pos (u32), cycles[4] (u64), h[4][2].  The block is split into
//     chunks of at most 256 frames (the engine's); per chunk of L frames:
//       1. ring[pos + i] = x_i, out_i = x_i dry
//       2. per voice v < voice_count, in order: t = (float)L / (float)sr, cyc = (double)t rate_v,
//            inc = llrint(cyc / L 65536), D = lrintf((float)(delay_ms / 1000 sr)), md = (float)(depth_ms / 1000 sr),
//            if ((unsigned)md + 10 > D) D = (int)md + 10;  cutoff >= 16000: c1 = 1, c2 = 0, else
//            c2 = (float)exp(-TAU cutoff / sr), c1 = 1 - c2;  vol = wet db2lin(level_db),
//            vol_l = (float)(vol clamp(1 - pan, 0, 1)), vol_r = (float)(vol clamp(1 + pan, 0, 1));
//          per frame i, lc = cycles[v] + i inc:  ph = (float)(lc & 0xFFFF) / 65536,  w = (float)sin(ph TAU) md,
//            wf = (int)floor(w), fr = w - wf, src = pos + i - D - wf,  a = ring[src], b = ring[src - 1],
//            val = (a + (b - a) fr) vol,  h = h c2 + val c1,  out_i += h;
//          after the chunk cycles[v] += lrintf((float)(cyc 65536)).  Voices >= voice_count keep cycles and h.
//       3. pos += L
//   GAS_FX_PHASER  state: phase (f32), h[2], zm1[6][2].  Per block: dmin = (float)(min_hz / (sr / 2)), dmax likewise,
//       inc = (float)(TAU (float)(rate_hz / sr)); per frame: phase += inc, while (phase >= TAU) phase = (float)(phase - TAU),
//       d = dmin + (dmax - dmin) ((sin(phase) + 1) / 2), a1 = (1 - d) / (1 + d); per ear:
//       u = x + h feedback, stages j = 5 .. 0: y = u (-a1) + zm1[j], zm1[j] = y a1 + u, u = y;  h = u, out = x + u depth
//
// Mapping (parallel work on every wave, a serial lane only for what is recurrent):
//   chorus: CS sources per workgroup, the block's input rows and every voice's val staged in LDS.  (1) One wave per
//     (source, voice, 64-frame tile), a lane per frame: the LFO, the fractional read -- from LDS where the frame lies
//     in this block, else from the ring in HBM (a read reaches 9 .. R - F frames back, so it never meets this block's
//     positions) -- and val for both ears, all of the block's reads before any chain; (2) one lane per (source, voice)
//     runs the h chain over the block, both ears packed two-wide; (3) one thread per (source, frame) sums dry and the
//     voices in voice order and writes the row.  The block goes into the
//     ring last, after every read of the launch.  The chunk rule only changes inc and the cycle step, so one F = 512
//     block equals two F = 256 blocks bit for bit.
//   phaser: PS sources per workgroup, KP-frame tiles.  The LFO is computed a tile ahead: a lane per source walks the
//     serial f32 phase of the next tile while the current tile's allpass chains run, then all threads evaluate the
//     sines and a1 into LDS.  One lane per source runs the chain with both ears packed (they share a1): per frame the
//     12 dependent multiply / add operations of the six stages and the feedback.
// No FMA contraction: products and sums round like the engine's separate f32 operations.
#include <cmath>

#include "gas_internal.h"

#pragma clang fp contract(off)

namespace {

typedef float f2 __attribute__((ext_vector_type(2))); // (left, right)

constexpr double TAU = 6.283185307179586;
constexpr uint32_t CHUNK = 256; // [ENGINE] the chorus's processing chunk
constexpr uint32_t MAXF = 512;

__device__ __forceinline__ float db2lin_block(float db) {
	return (float)exp((double)db * 0.11512925464970228);
}

__device__ __forceinline__ double clamp01(double v) {
	return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}

__device__ __forceinline__ f2 ld2(const float *p) {
	const float2 v = *reinterpret_cast<const float2 *>(p);
	return f2{ v.x, v.y };
}

__device__ __forceinline__ void st2(float *p, f2 v) {
	*reinterpret_cast<float2 *>(p) = make_float2(v.x, v.y);
}

// ---------------------------------------------------------------------------------------------------------------
// GAS_FX_CHORUS
// ---------------------------------------------------------------------------------------------------------------
constexpr int CV = GAS_CHORUS_MAX_VOICES;
constexpr int CS = 2; // sources per workgroup
constexpr int CNT = 256; // 4 waves
constexpr int KC = 64; // frames per step-1 task (a wave's lane per frame)
constexpr int KH = 16; // frames of a chain lane's LDS reads ahead
constexpr int XROW = MAXF * 2 + 4; // LDS row of one source's staged block
constexpr int VROW = MAXF * 2 + 2; // LDS row of one (source, voice)'s block: chain lane l reads bank 2 l + 2 k

struct ChorusVoice { // per (source, voice), LDS
	uint32_t lc0[2], inc[2]; // low bits of cycles at each chunk's start, and the chunk's increment
	int d;
	float md, c1, c2;
	float vol[2];
};

struct ChorusSrc { // per source, LDS
	float *line; // nullptr: no source, or no line entered (never expected; its rows are written as zeros)
	uint32_t row, pos;
	int vc, out;
	float dry;
};

__global__ __launch_bounds__(CNT) void k_fx_chorus(gas_group_args g, gas_dev_state st, uint32_t F, uint32_t j, float mix_rate, float *__restrict__ rows_out) {
	__shared__ ChorusSrc src[CS];
	__shared__ ChorusVoice voice[CS * CV];
	__shared__ float xs[CS * XROW];
	__shared__ float vals[CS * CV * VROW];

	const int tid = threadIdx.x;
	const uint32_t e0 = blockIdx.x * CS;
	const uint32_t mask = st.chorus_mask;
	const double sr = (double)mix_rate;

	// block constants; lane (s, v) of wave 0 keeps its h chain in registers
	f2 h = { 0.0f, 0.0f };
	float *line = nullptr;
	bool chain = false;
	uint64_t cyc_end = 0;
	if (tid < CS * CV) {
		const int s = tid / CV, v = tid % CV;
		const uint32_t e = e0 + s;
		const uint32_t slot = e < g.n ? (g.slots ? g.slots[e] : g.slot_base + e) : 0;
		const int li = e < g.n ? st.mod_of[(size_t)j * st.dyn_stride + slot] : -1;
		if (li >= 0) {
			const gas_fx_mod_settings *P = st.mod_settings + slot;
			line = st.chorus_pool + (size_t)li * (GAS_CHORUS_HEADER + 2 * ((size_t)mask + 1));
			const int vc = P->chorus_voice_count[j];
			chain = v < vc;
			h = ld2(line + GAS_CHORUS_H + 2 * v);
			const uint64_t cycles = reinterpret_cast<const uint64_t *>(line + 2)[v];
			ChorusVoice cv;
			cyc_end = cycles;
			for (uint32_t c = 0; c < 2; c++) {
				const uint32_t L = F > c * CHUNK ? (F - c * CHUNK < CHUNK ? F - c * CHUNK : CHUNK) : 0;
				cv.lc0[c] = (uint32_t)cyc_end;
				cv.inc[c] = 0;
				if (L) {
					const float t = (float)L / (float)mix_rate;
					const double cyc = (double)t * (double)P->chorus_rate_hz[j][v];
					cv.inc[c] = (uint32_t)(long long)rint(cyc / (double)L * 65536.0);
					cyc_end += (uint64_t)(long)rintf((float)(cyc * 65536.0));
				}
			}
			long d = (long)rintf((float)((double)P->chorus_delay_ms[j][v] / 1000.0 * sr));
			const float md = (float)((double)P->chorus_depth_ms[j][v] / 1000.0 * sr);
			if ((long)(unsigned)md + 10 > d) {
				d = (int)md + 10;
			}
			cv.d = (int)d;
			cv.md = md;
			const float cut = P->chorus_cutoff_hz[j][v];
			cv.c2 = cut >= 16000.0f ? 0.0f : (float)exp(-TAU * (double)cut / sr);
			cv.c1 = cut >= 16000.0f ? 1.0f : 1.0f - cv.c2;
			const float vol = P->chorus_wet[j] * db2lin_block(P->chorus_level_db[j][v]);
			const double pan = (double)P->chorus_pan[j][v];
			cv.vol[0] = (float)((double)vol * clamp01(1.0 - pan));
			cv.vol[1] = (float)((double)vol * clamp01(1.0 + pan));
			voice[tid] = cv;
			if (v == 0) {
				ChorusSrc d0;
				d0.line = line;
				d0.row = g.rows ? g.rows[e] : e;
				d0.pos = reinterpret_cast<const uint32_t *>(line)[0];
				d0.vc = vc;
				d0.out = 1;
				d0.dry = P->chorus_dry[j];
				src[s] = d0;
			}
		} else if (v == 0) {
			src[s].line = nullptr;
			src[s].vc = 0;
			src[s].out = e < g.n;
		}
	}
	__syncthreads();

	// the block's input rows
	for (uint32_t idx = tid; idx < CS * F; idx += CNT) {
		const uint32_t s = idx / F, i = idx % F;
		if (src[s].line) {
			st2(xs + s * XROW + 2 * i, ld2(reinterpret_cast<const float *>(g.src) + ((size_t)src[s].row * F + i) * 2));
		}
	}
	__syncthreads();

	// 1. val for every (source, voice, frame, ear): a wave per (source, voice, KC-frame tile), all of the block's reads
	//    in flight before any chain starts
	const int lane = tid & 63, wave = tid >> 6;
	for (uint32_t task = wave; task < CS * CV * (F / KC); task += CNT / 64) {
		const int l = task % (CS * CV), s = l / CV, v = l % CV;
		const ChorusSrc &cs = src[s];
		if (cs.line && v < cs.vc) {
			const ChorusVoice &cv = voice[l];
			const int i = (int)(task / (CS * CV)) * KC + lane;
			const int c = i >= (int)CHUNK;
			const uint32_t lc = cv.lc0[c] + (uint32_t)(i - c * (int)CHUNK) * cv.inc[c];
			const float ph = (float)(lc & 0xFFFFu) / 65536.0f;
			const float w = (float)sin((double)ph * TAU) * cv.md;
			const int wf = (int)floorf(w);
			const float fr = w - (float)wf;
			const int r = i - cv.d - wf; // frame of a relative to the block's first (<= i - 9)
			const float *ring = cs.line + GAS_CHORUS_HEADER;
			const f2 a = r >= 0 ? ld2(xs + s * XROW + 2 * r) : ld2(ring + (size_t)((cs.pos + (uint32_t)r) & mask) * 2);
			const f2 b = r - 1 >= 0 ? ld2(xs + s * XROW + 2 * (r - 1)) : ld2(ring + (size_t)((cs.pos + (uint32_t)(r - 1)) & mask) * 2);
			const f2 vol = { cv.vol[0], cv.vol[1] };
			st2(vals + l * VROW + 2 * i, (a + (b - a) * fr) * vol);
		}
	}
	__syncthreads();
	// 2. the h chains, one lane per (source, voice): c1 val off the critical path, KH frames ahead
	if (chain) {
		const ChorusVoice &cv = voice[tid];
		float *pv = vals + tid * VROW;
		for (uint32_t k0 = 0; k0 < F; k0 += KH) {
			f2 val[KH];
#pragma unroll
			for (int k = 0; k < KH; k++) {
				val[k] = ld2(pv + 2 * (k0 + k)) * cv.c1;
			}
#pragma unroll
			for (int k = 0; k < KH; k++) {
				h = h * cv.c2 + val[k];
				st2(pv + 2 * (k0 + k), h);
			}
		}
	}
	__syncthreads();
	// 3. dry plus the voices in voice order, one thread per (source, frame)
	for (uint32_t idx = tid; idx < CS * F; idx += CNT) {
		const uint32_t s = idx / F, i = idx % F;
		const ChorusSrc &cs = src[s];
		if (cs.line) {
			f2 o = ld2(xs + s * XROW + 2 * i) * cs.dry;
			for (int v = 0; v < cs.vc; v++) {
				o = o + ld2(vals + (s * CV + v) * VROW + 2 * i);
			}
			st2(rows_out + ((size_t)(e0 + s) * F + i) * 2, o);
		} else if (cs.out) {
			st2(rows_out + ((size_t)(e0 + s) * F + i) * 2, f2{ 0.0f, 0.0f });
		}
	}

	// the block into the ring, after every read of it; then the state
	for (uint32_t idx = tid; idx < CS * F; idx += CNT) {
		const uint32_t s = idx / F, i = idx % F;
		const ChorusSrc &cs = src[s];
		if (cs.line) {
			st2(cs.line + GAS_CHORUS_HEADER + (size_t)((cs.pos + i) & mask) * 2, ld2(xs + s * XROW + 2 * i));
		}
	}
	if (chain) {
		const int v = tid % CV;
		st2(line + GAS_CHORUS_H + 2 * v, h);
		reinterpret_cast<uint64_t *>(line + 2)[v] = cyc_end;
	}
	if (tid < CS * CV && line && tid % CV == 0) {
		reinterpret_cast<uint32_t *>(line)[0] = src[tid / CV].pos + F;
	}
}

// ---------------------------------------------------------------------------------------------------------------
// GAS_FX_PHASER
// ---------------------------------------------------------------------------------------------------------------
constexpr int PS = 32; // sources per workgroup: lane s of wave 0 runs source s's chain, lane s of wave 1 its phase
constexpr int PNT = 256;
constexpr int KP = 64; // frames per tile
constexpr int PXROW = KP * 2 + 2; // LDS row of one source's tile: chain lane s reads bank 2 s + 2 k
constexpr int PHROW = KP + 1;

__global__ __launch_bounds__(PNT) void k_fx_phaser(gas_group_args g, gas_dev_state st, uint32_t F, uint32_t j, float mix_rate, float *__restrict__ rows_out) {
	__shared__ float xs[2][PS * PXROW];
	__shared__ float phs[2][PS * PHROW];
	__shared__ float a1s[PS * PHROW];
	__shared__ float dmin[PS], dspan[PS];
	__shared__ uint32_t rowof[PS];
	__shared__ int has[PS]; // 1: a bank; 0: an entry without one (never expected; zeros); -1: no entry

	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t e0 = blockIdx.x * PS;
	const double sr = (double)mix_rate;
	const uint32_t T = F / KP;

	// wave 0 lane s: the chain; wave 1 lane s: the phase
	float *bank = nullptr;
	float fb = 0.0f, depth = 0.0f, phase = 0.0f, inc = 0.0f;
	f2 h = { 0.0f, 0.0f }, z[6];
	for (int k = 0; k < 6; k++) {
		z[k] = h;
	}
	if (wave < 2 && lane < PS) {
		const uint32_t e = e0 + lane;
		const uint32_t slot = e < g.n ? (g.slots ? g.slots[e] : g.slot_base + e) : 0;
		const int bi = e < g.n ? st.mod_of[(size_t)j * st.dyn_stride + slot] : -1;
		if (bi >= 0) {
			const gas_fx_mod_settings *P = st.mod_settings + slot;
			bank = st.phaser_pool + (size_t)bi * GAS_PHASER_BANK_FLOATS;
			if (wave == 0) {
				fb = P->phaser_feedback[j];
				depth = P->phaser_depth[j];
				h = ld2(bank + 2);
				for (int k = 0; k < 6; k++) {
					z[k] = ld2(bank + 4 + 2 * k);
				}
				const float lo = (float)((double)P->phaser_range_min_hz[j] / (sr / 2.0));
				const float hi = (float)((double)P->phaser_range_max_hz[j] / (sr / 2.0));
				dmin[lane] = lo;
				dspan[lane] = hi - lo;
				rowof[lane] = g.rows ? g.rows[e] : e;
			} else {
				phase = bank[0];
				inc = (float)(TAU * (double)(float)((double)P->phaser_rate_hz[j] / sr));
			}
		}
		if (wave == 0) {
			has[lane] = bi >= 0 ? 1 : (e < g.n ? 0 : -1);
		}
	}
	__syncthreads();

	// stage tile tl's input rows into xs[tl & 1] (waves from `first` on)
	auto stage = [&](uint32_t tl, int first) {
		float *xb = xs[tl & 1];
		for (int idx = tid - 64 * first; idx < PS * KP / 2; idx += PNT - 64 * first) { // 16-byte pieces: 2 frames
			const int s = idx / (KP / 2), p = idx % (KP / 2);
			if (has[s] > 0) {
				const float4 v = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(g.src) + ((size_t)rowof[s] * F + tl * KP + 2 * p) * 2);
				float *d = xb + s * PXROW + 4 * p;
				st2(d, f2{ v.x, v.y });
				st2(d + 2, f2{ v.z, v.w });
			}
		}
	};
	// the serial phase walk of tile tl into phs[tl & 1] (wave 1)
	auto walk = [&](uint32_t tl) {
		if (bank) {
			float *pp = phs[tl & 1] + lane * PHROW;
			for (int k = 0; k < KP; k++) {
				phase = phase + inc;
				while ((double)phase >= TAU) {
					phase = (float)((double)phase - TAU);
				}
				pp[k] = phase;
			}
		}
	};

	stage(0, 0);
	if (wave == 1 && lane < PS) {
		walk(0);
	}
	__syncthreads();

	for (uint32_t tl = 0; tl < T; tl++) {
		// A. the LFO of the tile: a1 per (source, frame)
		const float *pp = phs[tl & 1];
		for (int idx = tid; idx < PS * KP; idx += PNT) {
			const int s = idx / KP, k = idx % KP;
			if (has[s] <= 0) {
				continue;
			}
			const float sn = (float)sin((double)pp[s * PHROW + k]);
			const float d = dmin[s] + dspan[s] * ((sn + 1.0f) / 2.0f);
			a1s[s * PHROW + k] = (1.0f - d) / (1.0f + d);
		}
		__syncthreads();
		// B. the chains of this tile (wave 0) | the next tile's phase walk (wave 1) and rows (waves 1 ..)
		if (wave == 0) {
			if (bank) {
				float *xr = xs[tl & 1] + lane * PXROW;
				const float *ar = a1s + lane * PHROW;
#pragma unroll 8
				for (int k = 0; k < KP; k++) {
					const float a1 = ar[k], na1 = -a1;
					const f2 x = ld2(xr + 2 * k);
					f2 u = x + h * fb;
#pragma unroll
					for (int q = 5; q >= 0; q--) {
						const f2 y = u * na1 + z[q];
						z[q] = y * a1 + u;
						u = y;
					}
					h = u;
					st2(xr + 2 * k, x + u * depth);
				}
			}
		} else if (tl + 1 < T) {
			if (wave == 1 && lane < PS) {
				walk(tl + 1);
			}
			stage(tl + 1, 1);
		}
		__syncthreads();
		// C. rows out
		const float *xb = xs[tl & 1];
		for (int idx = tid; idx < PS * KP / 2; idx += PNT) {
			const int s = idx / (KP / 2), p = idx % (KP / 2);
			if (has[s] >= 0) {
				const float *sp = xb + s * PXROW + 4 * p;
				const float4 v = has[s] ? make_float4(sp[0], sp[1], sp[2], sp[3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
				*reinterpret_cast<float4 *>(rows_out + ((size_t)(e0 + s) * F + tl * KP + 2 * p) * 2) = v;
			}
		}
		// xs[tl & 1] is restaged in step B of the next iteration, after its barrier A
	}

	if (bank && wave == 0) {
		st2(bank + 2, h);
		for (int k = 0; k < 6; k++) {
			st2(bank + 4 + 2 * k, z[k]);
		}
	} else if (bank && wave == 1) {
		bank[0] = phase;
	}
}

} // namespace

hipError_t gas_launch_fx_mod(hipStream_t stream, int kind, const gas_group_args &g, const gas_dev_state &st, uint32_t frames, uint32_t chain_pos, float mix_rate, gas_audio_frame *rows_out) {
	if (g.n == 0) {
		return hipSuccess;
	}
	if (frames % KC != 0 || frames % KP != 0 || frames == 0 || frames > MAXF || chain_pos >= GAS_MAX_EFFECTS) {
		return hipErrorInvalidValue;
	}
	float *out = reinterpret_cast<float *>(rows_out);
	if (kind == GAS_FX_CHORUS && st.chorus_pool) {
		hipLaunchKernelGGL(k_fx_chorus, dim3((g.n + CS - 1) / CS), dim3(CNT), 0, stream, g, st, frames, chain_pos, mix_rate, out);
	} else if (kind == GAS_FX_PHASER && st.phaser_pool) {
		hipLaunchKernelGGL(k_fx_phaser, dim3((g.n + PS - 1) / PS), dim3(PNT), 0, stream, g, st, frames, chain_pos, mix_rate, out);
	} else {
		return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
