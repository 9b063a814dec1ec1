// k_room_bands.hip -- gas_conv_ir_from_room_bands and gas_conv_ir_from_room_hrtf_bands: steps 2, 4 and 5 of the rule in
// include/gas_amd.h (gas_conv_ir_from_room_bands).  The band sums of step 1 are k_room_ir.hip's, one unchanged pass per
// band; the band filters of step 3 are built on the host in float64 (gas_room_bands_fill_filters).
// tests/room_bands_ref.py restates the rule in numpy.
//
// k_room_bands_combine: y[e][t] = sum_b sum_j F_b[j] u_b[e][t + D - j], h = (float)(level y).  With the rows reversed on
// the host (G_b[i] = F_b[L - 1 - i]) this is a correlation, y[t] = sum_i G_b[i] u_b[t - D + i], over a window that only
// moves forward.
// Shape (the wide form): one workgroup of 256 lanes per tile of 1792 output taps and channel.  Per band the workgroup
// stages the tile's input window, u_b[t0 - D .. t0 - D + TILE + Lp - 1), in LDS: this is where the int64 sum becomes
// float64 and meets exp(-(lambda_b k)) (step 2), once per window element and not once per product; an index outside
// [0, taps) stages 0, which is how the rule drops such terms.  A lane owns 7 consecutive outputs in registers and walks
// the filter row 16 taps at a time: 16 new window values from LDS join the 6 it carries over (lane stride 7 doubles =
// 14 banks, odd in units of a double, so the lanes of a group meet different bank pairs) and feed 112 fused
// multiply-adds, and the 16 filter values are the same in every lane, so they arrive through one scalar load.  Rows are
// padded with zeros to Lp, a multiple of 16; a product with a padded zero adds +0 to a finite sum.
// Order of summation, fixed: bands ascending, within a band i ascending, one accumulator per output.  No atomics: two
// runs give the same bits.  Every product is fused into its sum (fma), which the rule allows; B = 1 is one product with
// 1.0 and sums with +0, exact either way.
// Bound: float64 FMA issue (one wave64 v_fma_f64 occupies its SIMD for 4 cycles); one LDS read per 7 FMAs.
// LDS: (TILE + Lp - 1) 8 bytes, 16 KiB at L = 255 and 46 KiB at L = 4095, so at least three workgroups share a CU.
// The narrow form: below 2^19 outputs (channels taps) seven outputs per lane leave most of the card idle -- a one-second
// stereo IR is 54 workgroups for 256 CUs, and each lane's chain of 7 B Lp dependent-issue FMAs is the kernel's time -- so
// the same kernel runs with one output per lane and tiles of 256 taps: seven times the lanes, a seventh of the chain, one
// LDS read per FMA (which an empty card affords) and a window staged for 256 taps instead of 1792.  Measured at 96 000
// outputs, B = 8, L = 1023: 0.32 ms -> 0.19 ms; a trip's loads, not its 16 FMAs, then set the time.  Both forms add the
// same terms in the same order, so which one ran cannot be read from the bits.
// Figures: profiles/room_bands_notes.md.
#include "gas_room_taps.h"

#include <cmath>

namespace {

constexpr uint32_t STEP = GAS_ROOM_BANDS_FILTER_STEP;
static_assert(GAS_ROOM_BANDS_TILE == 256u * 7u && GAS_ROOM_BANDS_SMALL_TILE == 256u && STEP == 16u, "k_room_bands_combine's register blocking");

template <uint32_t PER_LANE> // outputs per lane: 7 (the wide form) or 1 (the narrow form)
__global__ __launch_bounds__(256) void k_room_bands_combine(gas_room_bands_plan p, const long long *__restrict__ acc, const double *__restrict__ filt, float *__restrict__ out) {
	constexpr uint32_t TILE = 256u * PER_LANE;
	extern __shared__ double win[]; // TILE + Lp - 1
	const uint32_t tid = threadIdx.x, e = blockIdx.y;
	const long long t0 = (long long)blockIdx.x * TILE;
	const uint32_t W = TILE + p.Lp - 1u;
	double y[PER_LANE];
#pragma unroll
	for (uint32_t r = 0; r < PER_LANE; r++) {
		y[r] = 0.0;
	}
	for (uint32_t b = 0; b < p.bands; b++) {
		// step 2, while staging
		const long long *row = acc + ((size_t)b * p.channels + e) * p.taps;
		const double lam = p.lambda[b];
		if (b != 0) {
			__syncthreads(); // the previous band's window has been read by every lane
		}
		for (uint32_t i = tid; i < W; i += 256u) {
			const long long k = t0 - (long long)p.D + (long long)i;
			double u = 0.0;
			if (k >= 0 && k < (long long)p.taps) {
				u = (double)row[k] * (1.0 / GAS_ROOM_ONE);
				if (lam != 0.0) { // uniform; at 0 g is exactly 1
					u = u * exp(-(lam * (double)k));
				}
			}
			win[i] = u;
		}
		__syncthreads();
		// step 4
		const double *G = filt + (size_t)b * p.Lp;
		const double *x0 = win + tid * PER_LANE;
		double x[PER_LANE - 1 + STEP]; // the window slides through registers: PER_LANE - 1 values carried, 16 new per trip
#pragma unroll
		for (uint32_t m = 0; m < PER_LANE - 1; m++) {
			x[m] = x0[m];
		}
		for (uint32_t i0 = 0; i0 < p.Lp; i0 += STEP) {
#pragma unroll
			for (uint32_t m = PER_LANE - 1; m < PER_LANE - 1 + STEP; m++) {
				x[m] = x0[i0 + m]; // at most 255 PER_LANE + Lp - 16 + PER_LANE + 14 = TILE + Lp - 2 = W - 1
			}
#pragma unroll
			for (uint32_t s = 0; s < STEP; s++) {
				const double g = G[i0 + s];
#pragma unroll
				for (uint32_t r = 0; r < PER_LANE; r++) {
					y[r] = fma(g, x[r + s], y[r]);
				}
			}
#pragma unroll
			for (uint32_t m = 0; m < PER_LANE - 1; m++) {
				x[m] = x[m + STEP];
			}
		}
	}
	// step 5
#pragma unroll
	for (uint32_t r = 0; r < PER_LANE; r++) {
		const long long t = t0 + (long long)(tid * PER_LANE + r);
		if (t < (long long)p.taps) {
			out[(size_t)e * p.taps + (size_t)t] = (float)(p.level * y[r]);
		}
	}
}

} // namespace

// Step 3 -> host_filt [bands][Lp], row b reversed (G_b[i] = F_b[L - 1 - i]) and padded with zeros.
void gas_room_bands_fill_filters(const gas_room_bands &bands, double rate, const gas_room_bands_plan &p, double *g) {
	const uint32_t B = p.bands, L = p.L, D = p.D, Lp = p.Lp;
	for (size_t i = 0; i < (size_t)B * Lp; i++) {
		g[i] = 0.0;
	}
	if (B == 1) {
		g[0] = 1.0; // L = 1: delta_0
		return;
	}
	const double pi = 3.14159265358979323846;
	std::vector<double> lp((size_t)(B - 1) * L); // in the rule's order; reversed when the rows are written
	for (uint32_t i = 0; i + 1 < B; i++) {
		const double nu = (double)bands.crossover_hz[i] / rate;
		double *s = lp.data() + (size_t)i * L;
		double sum = 0.0;
		for (uint32_t j = 0; j < L; j++) {
			const double w = 0.42 - 0.5 * std::cos(2.0 * pi * (double)j / (double)(L - 1u)) + 0.08 * std::cos(4.0 * pi * (double)j / (double)(L - 1u));
			const double d = (double)j - (double)D;
			s[j] = w * (j == D ? 2.0 * nu : std::sin(2.0 * pi * nu * d) / (pi * d));
			sum += s[j];
		}
		for (uint32_t j = 0; j < L; j++) {
			s[j] = s[j] / sum;
		}
	}
	for (uint32_t b = 0; b < B; b++) {
		double *row = g + (size_t)b * Lp;
		for (uint32_t j = 0; j < L; j++) {
			const double hi = b + 1 < B ? lp[(size_t)b * L + j] : (j == D ? 1.0 : 0.0);
			const double lo = b > 0 ? lp[(size_t)(b - 1) * L + j] : 0.0;
			row[L - 1u - j] = hi - lo;
		}
	}
}

hipError_t gas_launch_room_bands_combine(hipStream_t stream, const gas_room_bands_plan &p, const long long *d_acc, const double *d_filt, float *d_out) {
	const bool wide = (uint64_t)p.channels * p.taps >= GAS_ROOM_BANDS_WIDE_FROM;
	const uint32_t tile = wide ? GAS_ROOM_BANDS_TILE : GAS_ROOM_BANDS_SMALL_TILE;
	const size_t lds = (size_t)(tile + p.Lp - 1u) * sizeof(double); // <= 47 096 bytes
	const dim3 grid((p.taps + tile - 1u) / tile, p.channels);
	if (wide) {
		hipLaunchKernelGGL(k_room_bands_combine<7>, grid, dim3(256), lds, stream, p, d_acc, d_filt, d_out);
	} else {
		hipLaunchKernelGGL(k_room_bands_combine<1>, grid, dim3(256), lds, stream, p, d_acc, d_filt, d_out);
	}
	return hipGetLastError();
}
