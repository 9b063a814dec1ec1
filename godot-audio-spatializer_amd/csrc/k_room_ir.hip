// k_room_ir.hip -- gas_conv_ir_from_room: the impulse response of a box room by the image method, built on the device.
// The rule is include/gas_amd.h's (gas_conv_ir_from_room), statement by statement in float64; tests/room_ir_ref.py
// restates it in numpy.
// Steps 1 and 2 (three points in the room's frame, d0, the candidate box) are a few dozen operations per call and run on
// the host (gas_room_ir_make_plan); the plan travels to the kernel by value.  A wall's reflectance to the power an image
// needs comes from per-axis tables of running products, 2 N_a + 1 doubles per axis, built on the host as well: pow() would
// tie the bits to a library.
// Shape: one lane per cell of the candidate box, m_z fastest, so a wave's lanes hold neighbouring images whose distances
// differ by about a room height each and whose taps therefore seldom collide.  A lane takes its cell (gas_room_cell with
// gas_room_cell_reflectance and gas_room_cell_image: the mask by |m|_1, R, the image) and per receiver deposits it
// (gas_room_deposit: one distance, two shares and two 64-bit integer adds without return on global memory); all are
// gas_room_taps.h's, shared with k_room_ir_hrtf below and with k_room_planes.hip.  No LDS: the two table values that
// are uniform over most of a wave and the third, read along the lanes, stay in cache.
// The sums are integers so that no order of arrival can change a bit; a second kernel scales them to float32
// [channels][taps], the layout gas_launch_conv_ir reads.
// Bound: 32 B of atomics per image and receiver against about sixty float64 operations; measured figures and the shell
// variant that would replace the box walk: profiles/room_ir_notes.md.
//
// k_room_ir_hrtf -- gas_conv_ir_from_room_hrtf: the same lattice heard through an HRIR set.  A lane takes its cell and its
// arrival at the one receiver (gas_room_cell, gas_room_arrival) and adds the direction of arrival in the listener's frame
// (the cell choice of k_calc_spatialization's hrtf_dir).  An image that reaches a tap is then spread by its whole wave:
// the wave walks its ballot of such lanes, takes each one's (k, a0, a1, dir) through lane reads, and per ear its 64 lanes
// stride over the hrir_taps + 1 taps of the HRIR shifted by the fractional delay, so one wave instruction adds to 64
// consecutive int64 (512 contiguous bytes) without return.  Nothing crosses a wave: no LDS, no barrier, and a lane that
// fails a mask stays for the spreading instead of returning.  Bound: up to 2 (hrir_taps + 1) adds of 8 bytes per image,
// 514 at 256 taps against 4 above; figures: profiles/room_brir_notes.md.  tests/room_brir_ref.py restates the rule in numpy.
// FMA contraction is off for the whole unit, host plan included: gas_room_taps.h sets it.
#include "gas_room_taps.h"

namespace {

__global__ __launch_bounds__(256) void k_room_ir(gas_room_ir_plan p, const double *__restrict__ tables, unsigned long long *__restrict__ acc) {
	const uint32_t id = blockIdx.x * 256u + threadIdx.x;
	if (id >= p.cells) {
		return;
	}
	// step 3
	int m[3];
	uint32_t at[3];
	if (!gas_room_cell(p, id, m, at)) {
		return;
	}
	const double R = gas_room_cell_reflectance(p, at, tables);
	if (!(R > 0.0)) {
		return; // every share would quantise to 0
	}
	double img[3];
	gas_room_cell_image(p, m, img);
	// steps 4 and 5
	for (uint32_t e = 0; e < p.channels; e++) {
		gas_room_deposit(img, p.e[e], R, p.d0, p.c, p.rate, p.taps, acc + (size_t)e * p.taps);
	}
}

// step 6
__global__ __launch_bounds__(256) void k_room_ir_scale(const long long *__restrict__ acc, uint32_t n, double level, float *__restrict__ out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < n) {
		out[i] = (float)(level * (double)acc[i] * (1.0 / GAS_ROOM_ONE));
	}
}

// One lane's value in every lane of the wave; src is the same in all of them and names a lane that is active.
__device__ __forceinline__ double wave_read(double v, int src) {
	return __shfl(v, src, 64);
}

__global__ __launch_bounds__(256) void k_room_ir_hrtf(gas_room_ir_plan p, gas_room_ir_frames fr, const double *__restrict__ tables, const float *__restrict__ hrir, uint32_t n_az, uint32_t n_el, uint32_t hrir_taps, unsigned long long *__restrict__ acc) {
	const uint32_t id = blockIdx.x * 256u + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	// phase 1: this lane's image; `hit` when it reaches a tap.  No lane leaves before the wave has spread its hits.
	bool hit = false;
	double a0 = 0.0, a1 = 0.0;
	int k = 0;
	uint32_t dir = 0;
	if (id < p.cells) {
		// step 1 (steps 1 - 3 of gas_conv_ir_from_room)
		int m[3];
		uint32_t at[3];
		if (gas_room_cell(p, id, m, at)) {
			const double R = gas_room_cell_reflectance(p, at, tables);
			double w[3];
			gas_room_cell_image(p, m, w);
#pragma unroll
			for (int a = 0; a < 3; a++) {
				w[a] = w[a] - p.e[0][a];
			}
			// step 2; an image with R == 0 stays out (every share would quantise to 0)
			if (gas_room_arrival(sqrt(gas_room_len2(w[0], w[1], w[2])), R, p.d0, p.c, p.rate, p.taps, k, a0, a1) && R > 0.0) { // taps <= 2^20: k fits an int
				hit = true;
				// step 3: into the global frame, then into the listener's
				double g[3], q[3];
#pragma unroll
				for (int a = 0; a < 3; a++) {
					g[a] = fr.B[a][0] * w[0] + fr.B[a][1] * w[1] + fr.B[a][2] * w[2];
				}
#pragma unroll
				for (int a = 0; a < 3; a++) {
					q[a] = fr.L[0][a] * g[0] + fr.L[1][a] * g[1] + fr.L[2][a] * g[2];
				}
				const double two_pi = 6.2831853071795864769252867666;
				const double az = atan2(q[0], -q[2]);
				const double flat = sqrt(q[0] * q[0] + q[2] * q[2]);
				const double el = atan2(q[1], flat);
				long long ai = llround(az / two_pi * n_az);
				ai = ((ai % (long long)n_az) + (long long)n_az) % (long long)n_az;
				long long ei = n_el > 1 ? llround((el + two_pi / 4) / (two_pi / 2) * (n_el - 1)) : 0;
				ei = ei < 0 ? 0 : (ei > (long long)n_el - 1 ? (long long)n_el - 1 : ei);
				dir = (uint32_t)(ei * n_az + ai); // < n_az n_el
			}
		}
	}
	// phase 2 (step 4): every lane of the wave is here, so the ballot and the lane reads see all 64
	unsigned long long live = __ballot(hit);
	while (live != 0) {
		const int src = __ffsll(live) - 1;
		live &= live - 1;
		const double b0 = wave_read(a0, src), b1 = wave_read(a1, src);
		const long long kk = __shfl(k, src, 64); // -1 .. taps - 1
		const size_t set = (size_t)__shfl((int)dir, src, 64) * 2u;
		for (uint32_t e = 0; e < 2; e++) {
			const float *H = hrir + (set + e) * hrir_taps;
			unsigned long long *row = acc + (size_t)e * p.taps;
			for (uint32_t j = lane; j <= hrir_taps; j += 64u) {
				const long long t = kk + (long long)j;
				if (t < 0 || t >= (long long)p.taps) {
					continue;
				}
				const double hj = j < hrir_taps ? (double)H[j] : 0.0;
				const double hp = j > 0 ? (double)H[j - 1] : 0.0;
				const long long q = llrint((b0 * hj + b1 * hp) * GAS_ROOM_ONE); // |.| <= 4 v 2^32 <= 2^34
				if (q != 0) {
					atomicAdd(row + t, (unsigned long long)q); // result unused: the no-return form; a negative q wraps as the sum of int64 does
				}
			}
		}
	}
}

// basis^T v, each sum in row order
void to_room_frame(const float basis[3][3], const double v[3], double out[3]) {
	for (int a = 0; a < 3; a++) {
		out[a] = (double)basis[0][a] * v[0] + (double)basis[1][a] * v[1] + (double)basis[2][a] * v[2];
	}
}

} // namespace

bool gas_room_ir_make_plan(const gas_room_ir &d, uint32_t channels, uint32_t taps, float rate, gas_room_ir_plan &p) {
	const gas_room &room = d.room;
	// step 1
	double rs[3], rl[3], rr[3], l[3], r[3];
	for (int a = 0; a < 3; a++) {
		rs[a] = (double)d.source[a] - (double)room.origin[a];
		rl[a] = (double)d.listener.origin[a] - (double)room.origin[a];
		rr[a] = (double)d.listener.basis[a][0];
		p.h[a] = (double)room.half_extent[a];
	}
	to_room_frame(room.basis, rs, p.s);
	to_room_frame(room.basis, rl, l);
	to_room_frame(room.basis, rr, r);
	for (int a = 0; a < 3; a++) {
		if (!(std::fabs(p.s[a]) <= p.h[a]) || !(std::fabs(l[a]) <= p.h[a])) {
			return false;
		}
	}
	const double half = (double)d.ear_spacing / 2.0;
	if (!gas_room_receivers(p.s, l, r, half, channels, p.d0, p.e)) {
		return false;
	}
	p.c = (double)room.speed_of_sound;
	p.rate = (double)rate;
	p.level = (double)room.level;
	// step 2
	const double reach = p.c * (double)taps / p.rate + p.d0 + (channels == 2 ? half : 0.0);
	double cells = 1.0;
	for (int a = 0; a < 3; a++) {
		double n = std::floor(reach / (2.0 * p.h[a])) + 1.0;
		if (d.max_order != 0 && n > (double)d.max_order) {
			n = (double)d.max_order;
		}
		if (!(n <= 134217728.0)) { // 2^27: one axis alone is past the cap (and a float64 that is no uint32 is never converted)
			return false;
		}
		p.N[a] = (uint32_t)n;
		cells *= 2.0 * n + 1.0; // three factors below 2^29: exact enough to compare, and exact whenever it is below 2^53
	}
	if (cells > (double)GAS_ROOM_IR_MAX_CELLS) {
		return false;
	}
	p.cells = (uint32_t)cells;
	p.min_order = d.min_order;
	p.max_order = d.max_order;
	p.channels = channels;
	p.taps = taps;
	return true;
}

hipError_t gas_launch_room_ir_scale(hipStream_t stream, const long long *d_acc, uint32_t n, double level, float *d_out) {
	hipLaunchKernelGGL(k_room_ir_scale, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_acc, n, level, d_out);
	return hipGetLastError();
}

size_t gas_room_ir_table_doubles(const gas_room_ir_plan &p) {
	return (size_t)(2u * p.N[0] + 1u) + (2u * p.N[1] + 1u) + (2u * p.N[2] + 1u);
}

void gas_room_ir_fill_tables(const gas_room_ir &d, const gas_room_ir_plan &p, double *t) {
	for (int a = 0; a < 3; a++) {
		const double neg = (double)d.room.reflectance[2 * a], pos = (double)d.room.reflectance[2 * a + 1];
		const uint32_t n = p.N[a];
		t[n] = 1.0; // index m + n; m = 0 meets no wall
		for (uint32_t m = 1; m <= n; m++) { // step m of a path towards +a meets +a when m is odd, and the other way round
			t[n + m] = t[n + m - 1] * ((m & 1) ? pos : neg);
			t[n - m] = t[n - m + 1] * ((m & 1) ? neg : pos);
		}
		t += 2u * n + 1u;
	}
}

hipError_t gas_launch_room_ir(hipStream_t stream, const gas_room_ir_plan &p, const double *d_tables, long long *d_acc, float *d_out) {
	return gas_room_launch_sums(stream, d_acc, p.channels * p.taps, p.level, d_out, [&](unsigned long long *acc) {
		hipLaunchKernelGGL(k_room_ir, dim3((p.cells + 255u) / 256u), dim3(256), 0, stream, p, d_tables, acc);
		return hipGetLastError();
	});
}

hipError_t gas_launch_room_ir_hrtf(hipStream_t stream, const gas_room_ir_plan &p, const gas_room_ir &d, const double *d_tables, const float *d_hrir, uint32_t n_az, uint32_t n_el, uint32_t hrir_taps, long long *d_acc, float *d_out) {
	gas_room_ir_frames fr;
	for (int a = 0; a < 3; a++) {
		for (int b = 0; b < 3; b++) {
			fr.B[a][b] = (double)d.room.basis[a][b];
			fr.L[a][b] = (double)d.listener.basis[a][b];
		}
	}
	return gas_room_launch_sums(stream, d_acc, 2u * p.taps, p.level, d_out, [&](unsigned long long *acc) {
		hipLaunchKernelGGL(k_room_ir_hrtf, dim3((p.cells + 255u) / 256u), dim3(256), 0, stream, p, fr, d_tables, d_hrir, n_az, n_el, hrir_taps, acc);
		return hipGetLastError();
	});
}
