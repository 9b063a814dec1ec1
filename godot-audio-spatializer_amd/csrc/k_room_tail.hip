// k_room_tail.hip -- gas_conv_ir_from_room_diffuse and gas_conv_ir_from_room_hrtf_diffuse: steps 1 and 3 - 6 of the rule
// in include/gas_amd.h (gas_conv_ir_from_room_diffuse).  The specular band sums of step 2 are k_room_ir.hip's, one
// unchanged pass per band for an IR of K1 taps; step 7 is k_room_bands.hip's combine over what this kernel writes.
// Step 3's decay constants (mu_b, s0) are a few dozen operations per call and are made on the host
// (gas_room_tail_make_plan); the plan travels to the kernel by value.  tests/room_tail_ref.py restates the rule in numpy.
//
// k_room_tail.  Shape: one lane per tap k of one ear, 256 lanes per workgroup, the ear in blockIdx.y.  A lane hashes its
// (seed, e, k) once (step 4) and keeps xi and f in registers; they are shared by all bands.  Step 5 needs the product
// a_b[k - 1] f[k - 1] of the tap below: the lane below has it in a register, so it comes through one wave shuffle per
// band (two 32-bit lane moves), and only lane 0 of a wave, whose neighbour lives in another wave, hashes tap k - 1 and
// takes that tap's exp itself.  That costs every wave a second pass through exp with one lane live; neither LDS and a
// barrier per band nor a wave of 63 taps with a halo lane was tried against it.  No lane leaves before the band loop ends,
// so every shuffle sees all 64 lanes.
// Per band a lane takes one float64 exp, reads acc_b[e][k] when k < K1 and writes acc'_b[e][k]: 16 bytes streamed per
// band, ear and tap below K1 and 8 above, against one exp (some forty float64 operations).  No atomics, no LDS: two runs
// give the same bits.  Below K0 a lane copies the sum (step 6 is exact there), and a wave wholly below K0 takes no exp.
// Bound: float64 issue, not memory -- 55 us for B = 8 at 2^20 taps and two ears is 2.4 TB/s of stores where plain stores
// reach 6, and about 130 float64 wave instructions per wave and band, the two trips through exp among them.
// Figures: profiles/room_tail_notes.md.
#include "gas_room_taps.h"

#include <algorithm>
#include <cmath>

// No FMA contraction, on the host or on the device: the rule fixes the order of the float64 operations.
#pragma clang fp contract(off)

namespace {

// Step 4: xi and f of tap k of ear e.
__device__ __forceinline__ void tail_noise(uint32_t seed, uint32_t e, uint32_t k, double &xi, double &f) {
	unsigned long long z = ((unsigned long long)seed << 32) | ((unsigned long long)e << 24) | (unsigned long long)k;
	z += 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	z ^= z >> 31;
	const int num = 2 * (int)((z & 0xffffu) + ((z >> 16) & 0xffffu) + ((z >> 32) & 0xffffu)) - 196605;
	xi = (double)num / sqrt(65536.0 * 65536.0 - 1.0);
	f = ((double)(uint32_t)(z >> 48) + 0.5) / 65536.0;
}

// Step 5: a_b[e][k] from the tap's xi.
__device__ __forceinline__ double tail_arrival(const gas_room_tail_plan &p, double mu, uint32_t k, double xi) {
	const double r = p.d0 + p.c * (double)k / p.rate;
	return (p.s0 * exp(-(mu * r) / 2.0)) * xi;
}

__global__ __launch_bounds__(256) void k_room_tail(gas_room_tail_plan p, const long long *__restrict__ spec, long long *__restrict__ acc) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x, e = blockIdx.y;
	const uint32_t lane = threadIdx.x & 63u;
	const bool live = k < p.taps; // a lane past the end stays for the shuffles and touches no memory
	const bool mixes = live && k >= p.K0; // below K0 step 6 is the specular sum itself
	const bool edge = lane == 0 && mixes && k > 0; // the tap below belongs to another wave
	const bool work = __any(mixes); // uniform: a wave wholly below K0 copies its sums and takes no exp
	// step 1
	double ws = 0.0, wd = 1.0;
	if (mixes && k < p.K1) { // K0 <= k < K1
		const double x = (double)(k - p.K0) / (double)(p.K1 - p.K0);
		ws = sqrt(1.0 - x);
		wd = sqrt(x);
	}
	// step 4
	double xi, f, xi_lo = 0.0, f_lo = 0.0;
	tail_noise(p.seed, e, k, xi, f);
	if (edge) {
		tail_noise(p.seed, e, k - 1u, xi_lo, f_lo);
	}
	for (uint32_t b = 0; b < p.bands; b++) {
		const size_t row = (size_t)b * p.channels + e;
		const bool dead = (p.dead >> b) & 1u; // uniform
		const double mu = p.mu[b];
		// step 5
		const double a = dead || !work ? 0.0 : tail_arrival(p, mu, k, xi);
		double below = __shfl_up(a * f, 1u, 64); // a_b[k - 1] f[k - 1] wherever lane - 1 holds tap k - 1
		if (lane == 0) {
			below = edge && !dead ? tail_arrival(p, mu, k - 1u, xi_lo) * f_lo : 0.0; // tap 0 has no tap below
		}
		const double d = a * (1.0 - f) + below;
		// step 6
		if (live) {
			long long q;
			if (!mixes) {
				q = spec[row * p.K1 + k]; // K0 <= K1
			} else {
				q = llrint((wd * d) * GAS_ROOM_ONE);
				if (k < p.K1) {
					q += llrint(ws * (double)spec[row * p.K1 + k]);
				}
			}
			acc[row * p.taps + k] = q;
		}
	}
}

bool finite_not_negative(float v) {
	return v >= 0.0f && std::isfinite(v);
}

} // namespace

bool gas_room_tail_marks(const gas_room_tail &t, double rate, uint32_t taps, uint32_t &K0, uint32_t &K1) {
	if (!finite_not_negative(t.mix_time_s) || !finite_not_negative(t.fade_s) || !finite_not_negative(t.gain) || t.reserved[0] != 0 || t.reserved[1] != 0 || t.reserved[2] != 0 || t.reserved[3] != 0) {
		return false;
	}
	const long long k0 = std::min<long long>(taps, llrint(std::fmin((double)t.mix_time_s * rate, 2147483648.0)));
	const long long k1 = std::min<long long>(taps, k0 + llrint(std::fmin((double)t.fade_s * rate, 2147483648.0)));
	K0 = (uint32_t)k0;
	K1 = (uint32_t)k1;
	return true;
}

bool gas_room_tail_make_plan(const gas_room_ir_plan &g, const gas_room_bands &bands, const gas_room_tail &t, uint32_t channels, uint32_t taps, uint32_t K0, uint32_t K1, gas_room_tail_plan &p) {
	// step 3
	const double pi = 3.14159265358979323846;
	const double V = 8.0 * g.h[0] * g.h[1] * g.h[2];
	const double A[3] = {4.0 * g.h[1] * g.h[2], 4.0 * g.h[0] * g.h[2], 4.0 * g.h[0] * g.h[1]};
	const double S = 2.0 * (A[0] + A[1] + A[2]);
	p.dead = 0;
	for (uint32_t b = 0; b < GAS_ROOM_MAX_BANDS; b++) {
		p.mu[b] = 0.0;
		if (b >= bands.n_bands) {
			continue;
		}
		double R[6];
		for (int w = 0; w < 6; w++) {
			R[w] = (double)bands.reflectance[b][w];
		}
		const double rho = (A[0] * (R[0] * R[0] + R[1] * R[1]) + A[1] * (R[2] * R[2] + R[3] * R[3]) + A[2] * (R[4] * R[4] + R[5] * R[5])) / S;
		if (rho == 0.0) {
			p.dead |= 1u << b;
		} else {
			p.mu[b] = -std::log(rho) * S / (4.0 * V);
		}
	}
	p.s0 = (double)t.gain * std::sqrt(((4.0 * pi * g.c) * (g.d0 * g.d0)) / (V * g.rate));
	if (!(p.s0 <= GAS_ROOM_TAIL_S0_MAX)) { // or not finite: |q| stays below 2^44
		return false;
	}
	p.K0 = K0;
	p.K1 = K1;
	p.d0 = g.d0;
	p.c = g.c;
	p.rate = g.rate;
	p.seed = t.seed;
	p.bands = bands.n_bands;
	p.channels = channels;
	p.taps = taps;
	return true;
}

hipError_t gas_launch_room_tail(hipStream_t stream, const gas_room_tail_plan &p, const long long *d_spec, long long *d_acc) {
	hipLaunchKernelGGL(k_room_tail, dim3((p.taps + 255u) / 256u, p.channels), dim3(256), 0, stream, p, d_spec, d_acc);
	return hipGetLastError();
}
