// k_fx_filter.hip -- the engine's AudioEffectFilter at any slope, and AudioEffectBandLimitFilter, as a stage of a staged
// effect chain (rows in -> dense rows out), settings from gas_fx_filter_settings by chain position, read
// once per block (coefficients snapped, no ramp):
//
//   GAS_FX_FILTER  [ENGINE] AudioEffectFilterInstance::process over AudioFilterSW.  NOT pinned against the engine's
//     source (a recollection, like SURVEY.md Appendix B).  Per block set_cutoff, set_gain, set_resonance,
//     set_stages(db + 1); all four processors of both ears take the same coefficients; every frame then runs through
//     processors 0 .. stages - 1 of its ear with process_one (gas_biquad.h's operation order).  Processors from `stages`
//     up are not run and keep their history.  The bank holds [stage 4][a1, a2, b1, b2][ear 2] floats.
//
// Geometry (wave64, NT = 256 threads): one DPP quad per (source, ear), lane s of the quad owns processor s, so a wave
// carries 8 sources and a workgroup S = 32.  The cascade is a software pipeline across the quad: at step t lane s runs
// frame t - s, its input lane s - 1's output of the step before, fetched with one quad permute (no LDS, no barrier);
// lane 0 reads the row.  Lanes from `stages` up only hand the value on, with the same one-step delay, so lane 3 always
// holds the finished frame t - 3 and writes it: the control flow is the same for every slope (a wave mixes quads of
// different `db`), a block is F + 3 steps of one process_one each, and the serial chain is as long as the one-stage
// kernel's instead of four times that.  The pipeline fills and drains inside the block (lanes idle while their frame
// index is outside 0 .. F - 1), so the state between blocks is exactly the engine's and one block of 512 frames is
// bitwise two of 256.
// The rows are staged through LDS in [S x KF frames] tiles with coalesced 16-byte loads by all threads, the next tile's
// loads in flight during the current one (as k_fx_eq.hip does).  The result goes back into the tile it came from;
// three tile buffers, because lane 3 still writes the last three frames of tile n - 1 while tile n runs: tile n - 1 is
// stored to the rows after tile n's steps, and its buffer is refilled only two tiles later.
// Row stride 34 floats: the 16 quads of a wave read 16 different banks.
// No FMA contraction: the f64 coefficient preparation and the f32 recurrence round like the engine's C++.
#include <cmath>

#include "gas_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256; // threads per workgroup
constexpr int S = NT / 8; // sources per workgroup: 4 stages x 2 ears each
constexpr int KF = 16; // frames per staged tile
constexpr int COLS = KF * 2; // floats of one source per tile (interleaved ears)
constexpr int ROW = COLS + 2; // LDS tile row stride in floats
constexpr int PARTS = COLS / 4; // 16-byte pieces of one source's tile row
constexpr int FILL = 3; // steps the pipeline needs to fill / drain
static_assert(S * PARTS == NT, "one staging load per thread and tile");
static_assert(KF > FILL, "lane 3 writes into the current tile and the one before");

struct Coeffs {
	float b0, b1, b2, a1, a2;
};

// [ENGINE] AudioFilterSW::prepare_coefficients for the modes AudioEffectFilter's subclasses select, `stages` cascaded
// stages.  gas_biquad.h's filter_coeffs / highshelf_coeffs are this at stages = 1, operation for operation (the 6 dB
// kinds 1 and 4 .. 8 give the same bits); the stage correction of Q and gain is the oracle's (gaso_highshelf_coeffs,
// SURVEY.md Appendix B): after the mode's Q tweak and the gain clamp, before alpha.  f64 arithmetic, members stored
// f32, then normalised by a0 with the feedback terms negated.
__device__ inline Coeffs staged_filter_coeffs(int type, float sampling_rate, float cutoff_hz, float resonance, float gain_lin, int stages) {
	Coeffs c;
	double a0;
	if (type == GAS_FILTER_BANDLIMIT) {
		// [ENGINE] AudioEffectBandLimitFilter as recalled: `resonance` is the band's other edge, the centre the mean of
		// the two, the bandwidth in octaves between centre and edge; RBJ's constant-peak band-pass over the raw centre
		const double hi = resonance;
		const double center = ((double)cutoff_hz + (double)resonance) / 2.0;
		const double bw = (log(center) - log(hi)) / 0.6931471805599453;
		const double omega = 6.2831853071795864769252867666 * center / (double)sampling_rate;
		const double sin_v = sin(omega);
		const double cos_v = cos(omega);
		const double alpha = sin_v * sinh(0.6931471805599453 / 2.0 * bw * omega / sin_v);
		a0 = 1.0 + alpha;
		c.b0 = (float)alpha;
		c.b1 = 0.0f;
		c.b2 = (float)(-alpha);
		c.a1 = (float)(-2.0 * cos_v);
		c.a2 = (float)(1.0 - alpha);
	} else {
		int sr_limit = (int)(sampling_rate / 2) + 512;
		double final_cutoff = ((double)cutoff_hz > sr_limit) ? (double)sr_limit : (double)cutoff_hz;
		if (final_cutoff < 1) {
			final_cutoff = 1;
		}
		double omega = 6.2831853071795864769252867666 * final_cutoff / (double)sampling_rate;
		double sin_v = sin(omega);
		double cos_v = cos(omega);
		double Q = resonance;
		if (Q <= 0.0) {
			Q = 0.0001;
		}
		if (type == GAS_FILTER_BANDPASS) {
			Q *= 2.0;
		}
		double tmpgain = gain_lin;
		if (tmpgain < 0.001) {
			tmpgain = 0.001;
		}
		if (stages > 1) {
			Q = (Q > 1.0 ? pow(Q, 1.0 / stages) : Q);
			tmpgain = pow(tmpgain, 1.0 / (stages + 1));
		}
		double alpha = sin_v / (2 * Q);
		a0 = 1.0 + alpha;
		switch (type) {
			case GAS_FILTER_LOWPASS:
				c.b0 = (float)((1.0 - cos_v) / 2.0);
				c.b1 = (float)(1.0 - cos_v);
				c.b2 = (float)((1.0 - cos_v) / 2.0);
				c.a1 = (float)(-2.0 * cos_v);
				c.a2 = (float)(1.0 - alpha);
				break;
			case GAS_FILTER_HIGHPASS:
				c.b0 = (float)((1.0 + cos_v) / 2.0);
				c.b1 = (float)(-(1.0 + cos_v));
				c.b2 = (float)((1.0 + cos_v) / 2.0);
				c.a1 = (float)(-2.0 * cos_v);
				c.a2 = (float)(1.0 - alpha);
				break;
			case GAS_FILTER_BANDPASS:
				c.b0 = (float)(alpha * sqrt(Q + 1));
				c.b1 = 0.0f;
				c.b2 = (float)(-alpha * sqrt(Q + 1));
				c.a1 = (float)(-2.0 * cos_v);
				c.a2 = (float)(1.0 - alpha);
				break;
			case GAS_FILTER_NOTCH:
				c.b0 = 1.0f;
				c.b1 = (float)(-2.0 * cos_v);
				c.b2 = 1.0f;
				c.a1 = (float)(-2.0 * cos_v);
				c.a2 = (float)(1.0 - alpha);
				break;
			default: { // the shelves
				double tmpq = sqrt(Q);
				if (tmpq <= 0) {
					tmpq = 0.001;
				}
				double beta = sqrt(tmpgain) / tmpq;
				if (type == GAS_FILTER_LOWSHELF) {
					a0 = (tmpgain + 1.0) + (tmpgain - 1.0) * cos_v + beta * sin_v;
					c.b0 = (float)(tmpgain * ((tmpgain + 1.0) - (tmpgain - 1.0) * cos_v + beta * sin_v));
					c.b1 = (float)(2.0 * tmpgain * ((tmpgain - 1.0) - (tmpgain + 1.0) * cos_v));
					c.b2 = (float)(tmpgain * ((tmpgain + 1.0) - (tmpgain - 1.0) * cos_v - beta * sin_v));
					c.a1 = (float)(-2.0 * ((tmpgain - 1.0) + (tmpgain + 1.0) * cos_v));
					c.a2 = (float)((tmpgain + 1.0) + (tmpgain - 1.0) * cos_v - beta * sin_v);
				} else { // GAS_FILTER_HIGHSHELF
					a0 = (tmpgain + 1.0) - (tmpgain - 1.0) * cos_v + beta * sin_v;
					c.b0 = (float)(tmpgain * ((tmpgain + 1.0) + (tmpgain - 1.0) * cos_v + beta * sin_v));
					c.b1 = (float)(-2.0 * tmpgain * ((tmpgain - 1.0) + (tmpgain + 1.0) * cos_v));
					c.b2 = (float)(tmpgain * ((tmpgain + 1.0) + (tmpgain - 1.0) * cos_v - beta * sin_v));
					c.a1 = (float)(2.0 * ((tmpgain - 1.0) - (tmpgain + 1.0) * cos_v));
					c.a2 = (float)((tmpgain + 1.0) - (tmpgain - 1.0) * cos_v - beta * sin_v);
				}
			} break;
		}
	}
	c.b0 = (float)((double)c.b0 / a0);
	c.b1 = (float)((double)c.b1 / a0);
	c.b2 = (float)((double)c.b2 / a0);
	c.a1 = (float)((double)c.a1 / (0.0 - a0));
	c.a2 = (float)((double)c.a2 / (0.0 - a0));
	return c;
}

// lane s of every quad takes lane s - 1's value (lane 0 its own, unused): quad_perm [0, 0, 1, 2]
__device__ __forceinline__ float from_stage_before(float v) {
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x90, 0xf, 0xf, false));
}

// One processor's history and the value it handed on last step.
struct Stage {
	float a1, a2, b1, b2, carry;
};

// STEPS steps of the pipeline, the first of them step t0 of the block.  xr: this (source, ear)'s column of the tile
// that holds frames t0 .. (read when READ), pr: the same of the tile before it.  EDGE: the pipeline is filling or
// draining, every lane checks its frame index; otherwise all frames t0 - 3 .. t0 + STEPS - 1 are inside the block.
template <bool EDGE, bool READ, int STEPS>
__device__ __forceinline__ void run_steps(const Coeffs &co, Stage &p, float *xr, float *pr, int s, bool on, uint32_t t0, uint32_t F) {
#pragma unroll
	for (int k = 0; k < STEPS; k++) {
		const float up = from_stage_before(p.carry);
		const float x = READ ? xr[2 * k] : 0.0f;
		const float in = s == 0 ? x : up;
		// [ENGINE] Processor::process_one
		const float y = in * co.b0 + p.b1 * co.b1 + p.b2 * co.b2 + p.a1 * co.a1 + p.a2 * co.a2;
		const bool live = EDGE ? (on && t0 + k - s < F) : on; // (unsigned: a frame index below 0 is out as well)
		if (live) {
			p.a2 = p.a1;
			p.b2 = p.b1;
			p.b1 = in;
			p.a1 = y;
		}
		p.carry = on ? y : in;
		if (s == 3 && (!EDGE || t0 + k - FILL < F)) { // frame t0 + k - 3 is through the cascade
			if (k >= FILL) {
				xr[2 * (k - FILL)] = p.carry;
			} else {
				pr[2 * (KF + k - FILL)] = p.carry;
			}
		}
	}
}

__global__ __launch_bounds__(NT) void k_fx_filter(gas_group_args g, gas_dev_state st, uint32_t F, uint32_t j, float mix_rate, float *__restrict__ rows_out) {
	__shared__ float tile[3][S * ROW];

	const int tid = threadIdx.x;
	const int s = tid & 3, ear = (tid >> 2) & 1, me = tid >> 3; // processor, ear, source within the workgroup
	const uint32_t e0 = blockIdx.x * S;
	const uint32_t e = e0 + me;
	const bool valid = e < g.n;
	const uint32_t ec = valid ? e : g.n - 1;
	const uint32_t slot = g.slots ? g.slots[ec] : g.slot_base + ec;
	const int32_t bank = st.flt_of[(size_t)j * st.dyn_stride + slot];
	float *state = valid && bank >= 0 ? st.flt_pool + (size_t)bank * GAS_FILTER_BANK_FLOATS + s * 8 + ear : nullptr;

	// block constants: the settings snapshot, the coefficients every processor of this playback snaps to
	const gas_fx_filter_settings *fs = st.flt_settings + slot;
	const int stages = fs->db[j] + 1;
	const Coeffs co = staged_filter_coeffs(fs->type[j], mix_rate, fs->cutoff_hz[j], fs->resonance[j], fs->gain[j], stages);
	const bool on = s < stages;
	Stage p = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
	if (state) {
		p.a1 = state[0];
		p.a2 = state[2];
		p.b1 = state[4];
		p.b2 = state[6];
	}

	// staging: this thread moves 16-byte piece tid % PARTS of source tid / PARTS of every tile
	const int lsrc = tid / PARTS, lpart = tid % PARTS;
	const uint32_t le = e0 + lsrc;
	const uint32_t lc = le < g.n ? le : g.n - 1;
	const uint32_t lrow = g.rows ? g.rows[lc] : lc;
	const float *ld = reinterpret_cast<const float *>(g.src) + (size_t)lrow * F * 2 + lpart * 4;
	float *sto = le < g.n ? rows_out + (size_t)le * F * 2 + lpart * 4 : nullptr;
	const int toff = lsrc * ROW + lpart * 4;
	float4 pre = *reinterpret_cast<const float4 *>(ld);

	const uint32_t n_tiles = F / KF;
	for (uint32_t tl = 0; tl <= n_tiles; tl++) { // the last round only drains the pipeline
		float *tb = tile[tl % 3];
		float *tp = tile[(tl + 2) % 3];
		if (tl < n_tiles) { // rows are 136 B apart: two 8-byte stores
			*reinterpret_cast<float2 *>(tb + toff) = make_float2(pre.x, pre.y);
			*reinterpret_cast<float2 *>(tb + toff + 2) = make_float2(pre.z, pre.w);
			if (tl + 1 < n_tiles) {
				pre = *reinterpret_cast<const float4 *>(ld + (size_t)(tl + 1) * COLS);
			}
		}
		__syncthreads();

		float *xr = tb + me * ROW + ear, *pr = tp + me * ROW + ear;
		if (tl == 0) {
			run_steps<true, true, KF>(co, p, xr, pr, s, on, 0, F);
		} else if (tl < n_tiles) {
			run_steps<false, true, KF>(co, p, xr, pr, s, on, tl * KF, F);
		} else {
			run_steps<true, false, FILL>(co, p, xr, pr, s, on, tl * KF, F);
		}
		__syncthreads();

		// the tile before this one is complete: rows out with the staging loads' own coalesced pattern
		if (tl > 0 && sto) {
			const float *t4 = tp + toff;
			*reinterpret_cast<float4 *>(sto + (size_t)(tl - 1) * COLS) = make_float4(t4[0], t4[1], t4[2], t4[3]);
		}
		// its buffer is refilled two rounds from now, after the next round's barriers
	}

	if (state && on) { // processors that did not run keep their history
		state[0] = p.a1;
		state[2] = p.a2;
		state[4] = p.b1;
		state[6] = p.b2;
	}
}

} // namespace

hipError_t gas_launch_fx_filter(hipStream_t stream, const gas_group_args &g, const gas_dev_state &st, uint32_t frames, uint32_t chain_pos, float mix_rate, gas_audio_frame *rows_out) {
	if (g.n == 0) {
		return hipSuccess;
	}
	if (frames % KF != 0 || frames < KF || chain_pos >= GAS_MAX_EFFECTS || !st.flt_pool) {
		return hipErrorInvalidValue;
	}
	hipLaunchKernelGGL(k_fx_filter, dim3((g.n + S - 1) / S), dim3(NT), 0, stream, g, st, frames, chain_pos, mix_rate, reinterpret_cast<float *>(rows_out));
	return hipGetLastError();
}
