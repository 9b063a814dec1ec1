// k_calc_er.hip -- SURVEY.md 8f: the producer of GAS_FX_EARLY_REFLECTIONS' parameters.  Image sources of a shoebox room
// up to second order for every source of a physics tick in one launch; the eight strongest become er_gain / er_delay
// of the slot's parameter row.  The rule is include/gas_amd.h's (gas_calc_early_reflections), statement by statement in
// float32; tests/er_rooms_ref.py restates it in float64.
// Shape: 32 lanes per source (two sources per wave, eight per workgroup).  Lane c < 24 owns candidate c; the room row,
// the pose and the listener are read at one address by the source's 32 lanes (one fetch, broadcast by the memory path);
// a lane's rank is a count over the 24 gains read with width-32 shuffles.  No LDS, no atomics, no branches: the tail and
// rule 2 only clear the gains / predicate the stores.
// (Loading one dword per lane and broadcasting 30 values with shuffles was measured slower: profiles/er_rooms_notes.md.)
// Bound: 12 B of pose and 96 B of room in, 64 (+ 64) B out per source.  Measured: 6.0 us at 8192 sources (the floor of a
// dispatch here, k_calc_spatialization takes 7.2), 22 us at 65536 (twice k_calc_spatialization's 10.3).
#include "gas_internal.h"

// No FMA contraction: the rule fixes the order of the float32 operations, and `dist - d0` cancels for images close to
// the direct path (see k_calc_spatialization.hip for the same choice).
#pragma clang fp contract(off)

namespace {

constexpr int ER_CANDIDATES = 24;
constexpr int ER_GROUP = 32; // lanes per source

// The 24 triples with 1 <= |m|_1 <= 2 in ascending (|m|_1, m_x, m_y, m_z), as (m_x + 2) | (m_y + 2) << 4 | (m_z + 2) << 8.
#define ER_M(x, y, z) (uint16_t)(((x) + 2) | (((y) + 2) << 4) | (((z) + 2) << 8))
__constant__ uint16_t ER_TRIPLES[ER_GROUP] = {
	ER_M(-1, 0, 0), ER_M(0, -1, 0), ER_M(0, 0, -1), ER_M(0, 0, 1), ER_M(0, 1, 0), ER_M(1, 0, 0), // first order
	ER_M(-2, 0, 0), ER_M(-1, -1, 0), ER_M(-1, 0, -1), ER_M(-1, 0, 1), ER_M(-1, 1, 0), //
	ER_M(0, -2, 0), ER_M(0, -1, -1), ER_M(0, -1, 1), ER_M(0, 0, -2), ER_M(0, 0, 2), ER_M(0, 1, -1), ER_M(0, 1, 1), ER_M(0, 2, 0), //
	ER_M(1, -1, 0), ER_M(1, 0, -1), ER_M(1, 0, 1), ER_M(1, 1, 0), ER_M(2, 0, 0), //
	ER_M(0, 0, 0), ER_M(0, 0, 0), ER_M(0, 0, 0), ER_M(0, 0, 0), ER_M(0, 0, 0), ER_M(0, 0, 0), ER_M(0, 0, 0), ER_M(0, 0, 0) // lanes 24 .. 31 own nothing
};
#undef ER_M

// one axis of rule 5: the image coordinate, and R times the walls the path meets on this axis (+a first, then -a)
__device__ __forceinline__ float image_axis(int m, float h, float s, float refl_neg, float refl_pos, float &R) {
	const int am = m < 0 ? -m : m;
	const int hi = (am + 1) >> 1, lo = am >> 1; // ceil, floor of |m| / 2: each 0 or 1
	const int p = m > 0 ? hi : lo, q = m > 0 ? lo : hi;
	R = R * (p ? refl_pos : 1.0f); // a factor of 1 leaves R as it is, bit for bit
	R = R * (q ? refl_neg : 1.0f);
	return (float)(2 * m) * h + ((am & 1) ? -s : s);
}

__global__ __launch_bounds__(256) void k_calc_er(const gas_room *__restrict__ rooms, const uint32_t *__restrict__ room_index, const gas_source_pose *__restrict__ poses, const gas_listener *__restrict__ listener, const uint32_t *__restrict__ slots, uint32_t n, uint32_t max_delay, float rate, gas_params *__restrict__ table, gas_er_taps *__restrict__ out_taps) {
	const uint32_t c = threadIdx.x & (ER_GROUP - 1);
	const uint32_t src = blockIdx.x * (256 / ER_GROUP) + threadIdx.x / ER_GROUP;
	const bool live = src < n; // the tail's lanes compute source n - 1 again and store nothing
	const uint32_t i = live ? src : n - 1;
	const uint32_t ri = room_index ? room_index[i] : 0u;
	const bool no_room = ri == GAS_ROOM_NONE;
	const gas_room *__restrict__ room = rooms + (no_room ? 0u : ri);
	const float *__restrict__ pos = poses[i].position;

	// rule 1: source and listener in the room's frame (basis_xform_inv of k_calc_spatialization.hip)
	float s[3], l[3], h[3];
	{
		float rs[3], rl[3];
#pragma unroll
		for (int a = 0; a < 3; a++) {
			rs[a] = pos[a] - room->origin[a];
			rl[a] = listener->origin[a] - room->origin[a];
			h[a] = room->half_extent[a];
		}
#pragma unroll
		for (int a = 0; a < 3; a++) {
			s[a] = room->basis[0][a] * rs[0] + room->basis[1][a] * rs[1] + room->basis[2][a] * rs[2];
			l[a] = room->basis[0][a] * rl[0] + room->basis[1][a] * rl[1] + room->basis[2][a] * rl[2];
		}
	}
	// rule 2
	bool outside = no_room;
#pragma unroll
	for (int a = 0; a < 3; a++) {
		outside = outside || fabsf(s[a]) > h[a] || fabsf(l[a]) > h[a];
	}
	// rule 3
	const float dx = s[0] - l[0], dy = s[1] - l[1], dz = s[2] - l[2];
	const float d0 = sqrtf(dx * dx + dy * dy + dz * dz);

	// rules 4 - 6 for this lane's candidate
	const uint32_t packed = ER_TRIPLES[c];
	const int mx = (int)(packed & 15u) - 2, my = (int)((packed >> 4) & 15u) - 2, mz = (int)((packed >> 8) & 15u) - 2;
	const uint32_t order = (uint32_t)((mx < 0 ? -mx : mx) + (my < 0 ? -my : my) + (mz < 0 ? -mz : mz));
	float R = 1.0f;
	const float ix = image_axis(mx, h[0], s[0], room->reflectance[0], room->reflectance[1], R) - l[0];
	const float iy = image_axis(my, h[1], s[1], room->reflectance[2], room->reflectance[3], R) - l[1];
	const float iz = image_axis(mz, h[2], s[2], room->reflectance[4], room->reflectance[5], R) - l[2];
	const float dist = sqrtf(ix * ix + iy * iy + iz * iz);
	float g = ((room->level * R) * d0) / dist;
	const float fr = ((dist - d0) / room->speed_of_sound) * rate;
	const float delay_raw = rintf(fr); // ties to even
	// !(delay_raw <= M) is delay_raw > M for every number and also drops a NaN (whose gain is not finite anyway)
	// !(g > 0): a NaN, and a zero of either sign becomes +0
	if (outside || order > room->max_order || !(dist > 0.0f) || !isfinite(g) || !(g > 0.0f) || !(delay_raw <= (float)max_delay)) {
		g = 0.0f;
	}
	const uint32_t delay = (g != 0.0f && delay_raw >= 1.0f) ? (uint32_t)delay_raw : 1u; // a dropped candidate is (0, 1)
	if (c >= ER_CANDIDATES) {
		g = -1.0f; // below every candidate: never counted, never among the first eight
	}

	// rule 7: rank = candidates with a larger gain + earlier candidates with the same gain -- a permutation of 0 .. 23
	uint32_t rank = 0;
#pragma unroll
	for (int j = 0; j < ER_CANDIDATES; j++) {
		const float gj = __shfl(g, j, ER_GROUP);
		rank += (gj > g || (gj == g && (uint32_t)j < c)) ? 1u : 0u;
	}
	if (live && c < ER_CANDIDATES && rank < GAS_ER_TAPS) {
		if (table) {
			gas_params *P = table + slots[i];
			P->er_gain[rank] = g;
			P->er_delay[rank] = delay;
		}
		if (out_taps) {
			out_taps[i].gain[rank] = g;
			out_taps[i].delay[rank] = delay;
		}
	}
}

} // namespace

hipError_t gas_launch_calc_er(hipStream_t stream, const gas_room *rooms, const uint32_t *room_index, const gas_source_pose *poses, const gas_listener *listener, const uint32_t *slots, uint32_t n, uint32_t max_delay, float rate, gas_params *table, gas_er_taps *out_taps) {
	if (n == 0) {
		return hipSuccess;
	}
	constexpr uint32_t per_wg = 256 / ER_GROUP;
	hipLaunchKernelGGL(k_calc_er, dim3((n + per_wg - 1) / per_wg), dim3(256), 0, stream, rooms, room_index, poses, listener, slots, n, max_delay, rate, table, out_taps);
	return hipGetLastError();
}
