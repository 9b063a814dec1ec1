// k_room_planes.hip -- gas_conv_ir_from_planes: the impulse response of a room bounded by up to 16 planes, by the image
// method over plane sequences, built on the device.  The rule is include/gas_amd.h's (gas_conv_ir_from_planes), statement
// by statement in float64; tests/room_planes_ref.py restates it in numpy.
// Step 1 (unit normals, source, receivers, d0) and the layout of the candidates are a few hundred operations per call and
// run on the host (gas_room_planes_make_plan); the plan, planes included, travels to the kernel by value and is read
// through the scalar cache wherever the index is uniform.
// Shape: one lane per candidate sequence.  The flat index decodes to an order and then to digits, most significant
// first, so neighbouring lanes share a prefix: they reflect the same images, fail the same `t > 0` and leave the image
// loop together.  A lane builds its up to eight images (step 3), then per receiver walks the path back from the receiver
// (step 4: one intersection and P - 1 face tests per reflection) and, for a valid path, deposits the last image as
// k_room_ir deposits a cell's (gas_room_taps.h's gas_room_deposit, step 5; the direct sound goes the same way).  The
// sums are integers, so no order of arrival can change a bit; k_room_ir's scaling kernel turns them into float32
// [channels][taps].
// No LDS, no barrier, no wave operation: a lane may return wherever its sequence is settled -- a void sequence, R == 0
// (every share would quantise to 0), or a prefix image further from every receiver than any tap reaches: reflecting a
// point that is inside a half-space moves it away from every point inside the room, so the images after it are further
// still.  That test leaves a whole tap of slack ((taps + 1) in far2), which no rounding of a distance comes near.
// The images and digits live in registers: every loop over the order has a compile-time bound and a guard, so nothing
// is indexed by a run-time value but the plan itself.  Bound: float64 VALU -- per sequence and receiver about
// K (12 + 6 (P - 1)) operations against at most 32 B of atomics; measured figures: profiles/room_planes_notes.md.
// FMA contraction is off for the whole unit, host plan included: gas_room_taps.h sets it.
#include "gas_room_taps.h"

namespace {

constexpr int MAX_K = GAS_ROOM_PLANES_MAX_ORDER;

__host__ __device__ __forceinline__ double dot3(const double n[3], const double x[3]) {
	return (n[0] * x[0] + n[1] * x[1]) + n[2] * x[2];
}

__global__ __launch_bounds__(256) void k_room_planes(gas_room_planes_plan p, unsigned long long *__restrict__ acc) {
	const uint32_t id = blockIdx.x * 256u + threadIdx.x;
	if (id >= p.candidates) {
		return;
	}
	if (id == 0 && p.direct) { // step 2's direct sound: nothing to reflect and nothing to validate
		for (uint32_t e = 0; e < p.channels; e++) {
			gas_room_deposit(p.s, p.e[e], 1.0, p.d0, p.c, p.rate, p.taps, acc + (size_t)e * p.taps);
		}
	}
	// the order, then the digits' value within it
	uint32_t K = p.lo, rem = id;
#pragma unroll
	for (int k = 2; k <= MAX_K; k++) {
		if ((uint32_t)k > p.lo && (uint32_t)k <= p.hi && id >= p.first[k]) {
			K = (uint32_t)k;
			rem = id - p.first[k];
		}
	}
	const uint32_t others = p.P > 1u ? p.P - 1u : 1u;
	// step 3
	double img[MAX_K][3];
	uint32_t q[MAX_K];
	double at[3] = {p.s[0], p.s[1], p.s[2]};
	double R = 1.0;
	uint32_t prev = 0;
#pragma unroll
	for (int i = 0; i < MAX_K; i++) {
		if ((uint32_t)i < K) {
			const uint32_t top = rem / p.pw[K - 1u - (uint32_t)i]; // the digits down to this one
			uint32_t qi = top; // the first digit: base P
			if (i > 0) {
				const uint32_t digit = top % others;
				qi = digit + (digit >= prev ? 1u : 0u); // base P - 1, past the plane before
			}
			prev = qi;
			const double n[3] = {p.n[qi][0], p.n[qi][1], p.n[qi][2]};
			const double t = dot3(n, at) - p.d[qi];
			if (!(t > 0.0)) {
				return; // void
			}
			const double t2 = 2.0 * t;
			at[0] = at[0] - t2 * n[0];
			at[1] = at[1] - t2 * n[1];
			at[2] = at[2] - t2 * n[2];
			R = R * p.refl[qi];
			if (!(R > 0.0)) {
				return; // every share would quantise to 0
			}
			bool far = true;
			for (uint32_t e = 0; e < p.channels; e++) {
				far = far && (gas_room_len2(at[0] - p.e[e][0], at[1] - p.e[e][1], at[2] - p.e[e][2]) > p.far2);
			}
			if (far) {
				return; // no image made from this one reaches a tap
			}
			img[i][0] = at[0];
			img[i][1] = at[1];
			img[i][2] = at[2];
			q[i] = qi;
		}
	}
	// steps 4 and 5
	for (uint32_t e = 0; e < p.channels; e++) {
		const double ear[3] = {p.e[e][0], p.e[e][1], p.e[e][2]};
		double pt[3] = {ear[0], ear[1], ear[2]};
		bool valid = true;
#pragma unroll
		for (int i = MAX_K - 1; i >= 0; i--) {
			if ((uint32_t)i < K && valid) {
				const uint32_t qi = q[i];
				const double n[3] = {p.n[qi][0], p.n[qi][1], p.n[qi][2]};
				const double a = dot3(n, pt) - p.d[qi];
				const double b = dot3(n, img[i]) - p.d[qi];
				if (!(a > 0.0)) {
					valid = false;
				} else {
					const double u = a / (a - b);
					pt[0] = pt[0] + u * (img[i][0] - pt[0]);
					pt[1] = pt[1] + u * (img[i][1] - pt[1]);
					pt[2] = pt[2] + u * (img[i][2] - pt[2]);
					for (uint32_t j = 0; j < p.P; j++) { // j is uniform: the plane comes through the scalar cache
						const bool inside = dot3(p.n[j], pt) - p.d[j] >= 0.0;
						valid = valid && (inside || j == qi);
					}
				}
			}
		}
		if (valid) {
			gas_room_deposit(at, ear, R, p.d0, p.c, p.rate, p.taps, acc + (size_t)e * p.taps);
		}
	}
}

} // namespace

bool gas_room_planes_make_plan(const gas_room_planes &d, uint32_t channels, uint32_t taps, float rate, gas_room_planes_plan &p) {
	// step 1
	p.P = d.n_planes;
	for (uint32_t j = 0; j < p.P; j++) {
		const double x = (double)d.planes[j].normal[0], y = (double)d.planes[j].normal[1], z = (double)d.planes[j].normal[2];
		const double len = std::sqrt(gas_room_len2(x, y, z));
		if (!(len >= 0.999) || !(len <= 1.001)) {
			return false;
		}
		p.n[j][0] = x / len;
		p.n[j][1] = y / len;
		p.n[j][2] = z / len;
		p.d[j] = (double)d.planes[j].offset;
		p.refl[j] = (double)d.planes[j].reflectance;
	}
	double l[3], r[3];
	for (int a = 0; a < 3; a++) {
		p.s[a] = (double)d.source[a];
		l[a] = (double)d.listener.origin[a];
		r[a] = (double)d.listener.basis[a][0];
	}
	const double half = (double)d.ear_spacing / 2.0;
	if (!gas_room_receivers(p.s, l, r, half, channels, p.d0, p.e)) {
		return false;
	}
	for (uint32_t j = 0; j < p.P; j++) {
		if (!(dot3(p.n[j], p.s) - p.d[j] > 0.0) || !(dot3(p.n[j], p.e[0]) - p.d[j] > 0.0) || !(dot3(p.n[j], p.e[1]) - p.d[j] > 0.0)) {
			return false;
		}
	}
	p.c = (double)d.speed_of_sound;
	p.rate = (double)rate;
	p.level = (double)d.level;
	const double reach = p.c * ((double)taps + 1.0) / p.rate + p.d0;
	p.far2 = reach * reach;
	// step 2: P (P - 1)^(K - 1) sequences of order K; (P - 1)^7 <= 15^7 < 2^28
	p.lo = d.min_order > 1u ? d.min_order : 1u;
	p.hi = d.max_order;
	uint64_t pw = 1, total = 0;
	for (uint32_t k = 0; k < GAS_ROOM_PLANES_MAX_ORDER; k++) {
		p.pw[k] = (uint32_t)pw;
		pw *= p.P - 1u;
	}
	for (uint32_t K = 0; K < GAS_ROOM_PLANES_MAX_ORDER + 2u; K++) {
		p.first[K] = 0;
	}
	for (uint32_t K = p.lo; K <= p.hi; K++) {
		p.first[K] = (uint32_t)total;
		total += (uint64_t)p.P * p.pw[K - 1u]; // below 2^32 each, eight of them
		if (total > GAS_ROOM_PLANES_MAX_CANDIDATES) {
			return false;
		}
	}
	p.first[p.hi + 1u] = (uint32_t)total;
	p.candidates = (uint32_t)total;
	p.direct = d.min_order == 0 ? 1u : 0u;
	p.channels = channels;
	p.taps = taps;
	return true;
}

hipError_t gas_launch_room_planes(hipStream_t stream, const gas_room_planes_plan &p, long long *d_acc, float *d_out) {
	return gas_room_launch_sums(stream, d_acc, p.channels * p.taps, p.level, d_out, [&](unsigned long long *acc) {
		if (p.candidates == 0) { // P == 1 with min_order > 1 has none: a lone plane reflects once
			return hipSuccess;
		}
		hipLaunchKernelGGL(k_room_planes, dim3((p.candidates + 255u) / 256u), dim3(256), 0, stream, p, acc);
		return hipGetLastError();
	});
}
