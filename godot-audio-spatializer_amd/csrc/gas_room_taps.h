// gas_room_taps.h -- what the room impulse response units (k_room_ir.hip, k_room_planes.hip, k_room_tail.hip,
// k_room_bands.hip) share, so that "a box as six planes is the box call" and "a delta HRIR set is the one-channel call"
// (include/gas_amd.h) hold because both roads run the same statements: the scale of the integer sums, steps 3 - 5 of
// gas_conv_ir_from_room on the device, and on the host the receivers of a plan and the launch sequence around an
// accumulating kernel.  Everything is float64 in the order the rule writes it.
// The device pieces are forced inline and pass their results through references to the caller's own locals: no struct is
// filled and carried, so a kernel's registers are what they were with the statements written out (k_room_planes: 120
// VGPRs, no scratch; profiles/room_family_notes.md).
#pragma once

#include "gas_internal.h"

#include <cmath>

// No FMA contraction, on the host or on the device, from here to the end of the including unit: the rule fixes the order
// of the float64 operations, and `dist - d0` cancels for images close to the direct path.
#pragma clang fp contract(off)

constexpr double GAS_ROOM_ONE = 4294967296.0; // 2^32: a share of 1 as an integer

// |(dx, dy, dz)|^2, summed in this order wherever a distance is taken.
__host__ __device__ __forceinline__ double gas_room_len2(double dx, double dy, double dz) {
	return dx * dx + dy * dy + dz * dz;
}

// The lattice cell `id` of a box plan (m_z fastest; id < p.cells): its m, its indices `at` into the three tables, and
// whether the order mask keeps it.  The helpers report; the kernel decides when a lane leaves.
__device__ __forceinline__ bool gas_room_cell(const gas_room_ir_plan &p, uint32_t id, int m[3], uint32_t at[3]) {
	const uint32_t wz = 2u * p.N[2] + 1u, wy = 2u * p.N[1] + 1u;
	at[2] = id % wz;
	const uint32_t rest = id / wz;
	at[1] = rest % wy;
	at[0] = rest / wy;
#pragma unroll
	for (int a = 0; a < 3; a++) {
		m[a] = (int)at[a] - (int)p.N[a];
	}
	const uint32_t order = (uint32_t)((m[0] < 0 ? -m[0] : m[0]) + (m[1] < 0 ? -m[1] : m[1]) + (m[2] < 0 ? -m[2] : m[2]));
	return !(order < p.min_order || (p.max_order != 0 && order > p.max_order));
}

// Step 3 of gas_conv_ir_from_room for a kept cell: the reflectance its walls leave, from the three tables.  It may be 0:
// every share would then quantise to 0.
__device__ __forceinline__ double gas_room_cell_reflectance(const gas_room_ir_plan &p, const uint32_t at[3], const double *__restrict__ tables) {
	const double *tx = tables, *ty = tx + (2u * p.N[0] + 1u), *tz = ty + (2u * p.N[1] + 1u);
	return (tx[at[0]] * ty[at[1]]) * tz[at[2]];
}

// ... and its image point in the room's frame.
__device__ __forceinline__ void gas_room_cell_image(const gas_room_ir_plan &p, const int m[3], double img[3]) {
#pragma unroll
	for (int a = 0; a < 3; a++) {
		img[a] = (double)(2 * m[a]) * p.h[a] + ((m[a] & 1) ? -p.s[a] : p.s[a]);
	}
}

// Step 4 of gas_conv_ir_from_room for an image at `dist` from a receiver: false when it reaches no tap (a NaN is dropped
// here); otherwise its two shares a0 and a1, in [0, 1] for R in [0, 1], belong to taps k and k + 1, k in -1 .. taps - 1.
// The comparisons are in double first, which keeps the conversion defined whatever comes.  K: the caller's integer, int
// or long long; taps <= 2^20 fits either.
template <class K>
__device__ __forceinline__ bool gas_room_arrival(double dist, double R, double d0, double c, double rate, uint32_t taps, K &k, double &a0, double &a1) {
	const double v = R * d0 / fmax(dist, d0);
	const double pos = (dist - d0) / c * rate;
	const double kf = floor(pos);
	const double f = pos - kf;
	if (!(kf >= -1.0) || !(kf < (double)taps)) {
		return false;
	}
	k = (K)kf;
	a0 = v * (1.0 - f);
	a1 = v * f;
	return true;
}

// Steps 4 and 5 of gas_conv_ir_from_room for one image and one receiver whose sums are `row` [taps]: the arrival, then
// its shares as integers in [0, 2^32], added without return.
__device__ __forceinline__ void gas_room_deposit(const double img[3], const double ear[3], double R, double d0, double c, double rate, uint32_t taps, unsigned long long *__restrict__ row) {
	long long k;
	double a0, a1;
	if (!gas_room_arrival(sqrt(gas_room_len2(img[0] - ear[0], img[1] - ear[1], img[2] - ear[2])), R, d0, c, rate, taps, k, a0, a1)) {
		return;
	}
	const unsigned long long q0 = (unsigned long long)llrint(a0 * GAS_ROOM_ONE);
	const unsigned long long q1 = (unsigned long long)llrint(a1 * GAS_ROOM_ONE);
	if (k >= 0 && q0 != 0) {
		atomicAdd(row + k, q0); // result unused: the no-return form
	}
	if (k + 1 < (long long)taps && q1 != 0) {
		atomicAdd(row + k + 1, q1);
	}
}

// The receivers of a plan, on the host: d0 from the source s to the listener l, and e -- both the listener for one
// channel, otherwise l -+ half r (r: column 0 of the listener's basis), all in the plan's frame.  False for d0 < 1e-3.
inline bool gas_room_receivers(const double s[3], const double l[3], const double r[3], double half, uint32_t channels, double &d0, double e[2][3]) {
	d0 = std::sqrt(gas_room_len2(s[0] - l[0], s[1] - l[1], s[2] - l[2]));
	for (int a = 0; a < 3; a++) {
		e[0][a] = channels == 1 ? l[a] : l[a] - half * r[a];
		e[1][a] = channels == 1 ? l[a] : l[a] + half * r[a];
	}
	return d0 >= 1e-3;
}

// What every gas_launch_room_* is, in stream order: zero d_acc [n], let `accumulate` launch the kernel that adds to it
// (it returns the launch's status, or hipSuccess when it has nothing to launch), scale the sums into d_out [n] f32.
template <class Accumulate>
inline hipError_t gas_room_launch_sums(hipStream_t stream, long long *d_acc, uint32_t n, double level, float *d_out, Accumulate accumulate) {
	hipError_t e = hipMemsetAsync(d_acc, 0, sizeof(long long) * n, stream);
	if (e != hipSuccess) {
		return e;
	}
	e = accumulate(reinterpret_cast<unsigned long long *>(d_acc));
	if (e != hipSuccess) {
		return e;
	}
	return gas_launch_room_ir_scale(stream, d_acc, n, level, d_out);
}
