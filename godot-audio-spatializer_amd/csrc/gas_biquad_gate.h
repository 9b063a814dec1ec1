// gas_biquad_gate.h -- which sources of a filter stage may take the lane-parallel scan form (k_shelf_scan.hip,
// k_hrtf_uni.hip's FLT branch) and which keep the engine-order serial loop.  Plain C, no HIP types: the kernels include
// it with GAS_GATE_FN = __host__ __device__, tests/test_filter_scan_gate_reference.py compiles it with gcc as it stands.
//
// The scan rounds differently from the serial loop and its error grows with the filter's CONDITIONING: a rounding error
// made in one lane travels through the feedback part 1 / A(z), A(z) = 1 - a1 z^-1 - a2 z^-2 (feedback terms stored
// negated), and comes out scaled by up to the peak gain of that all-pole part,  G = max over w of 1 / |A(e^jw)|.
// |a2| does not measure that (it is the pole radius squared for a complex pair only: an over-damped filter has two real
// poles whose product it is, and a complex pair at a small angle is a near-double pole next to z = 1 whatever its
// radius), so the gate bounds G itself, in closed form: with c = cos w,
//   |A|^2 = (1 + a1^2 + a2^2 + 2 a2) + 2 a1 (a2 - 1) c - 4 a2 c^2,
// a parabola in c whose minimum over [-1, 1] is at an end point, (1 - a1 - a2)^2 at w = 0 or (1 + a1 - a2)^2 at w = pi,
// or, when it opens upward (a2 < 0) and the stationary point c* = a1 (a2 - 1) / (4 a2) lies inside, at c*.
// The scan runs where the filter is stable and G <= GAS_SCAN_MAX_ALLPOLE_GAIN = 40; a float32 model of the scan puts its
// row error there below 7e-6 of the row's peak (DESIGN.md 3.5 (a) has the figures).  NaN coefficients fail every
// comparison and go serial.
#pragma once

#ifndef GAS_GATE_FN
#define GAS_GATE_FN
#endif

#define GAS_SCAN_MAX_ALLPOLE_GAIN 40.0f

// Both callers must decide alike for the same coefficients (the one-launch form is pinned bitwise to the two-launch
// form), whatever contraction mode the including file runs in: no FMA contraction in here.
GAS_GATE_FN static inline int gas_biquad_scan_allowed(float a1, float a2) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
	const float lim = 1.0f / (GAS_SCAN_MAX_ALLPOLE_GAIN * GAS_SCAN_MAX_ALLPOLE_GAIN); // smallest |A|^2 allowed
	const float abs_a1 = a1 < 0.0f ? -a1 : a1;
	if (!(a2 > -1.0f && a2 < 1.0f && abs_a1 < 1.0f - a2)) { // the stability triangle; NaN and infinities end here
		return 0;
	}
	const float e0 = (1.0f - a1 - a2) * (1.0f - a1 - a2); // w = 0
	const float e1 = (1.0f + a1 - a2) * (1.0f + a1 - a2); // w = pi
	float m = e0 < e1 ? e0 : e1;
	if (a2 < 0.0f) {
		const float c = a1 * (a2 - 1.0f) / (4.0f * a2);
		if (c >= -1.0f && c <= 1.0f) {
			const float lin = 2.0f * a1 * (a2 - 1.0f);
			const float v = (1.0f + a1 * a1 + a2 * a2 + 2.0f * a2) + lin * lin / (16.0f * a2); // |A|^2 at c*
			m = v < m ? v : m;
		}
	}
	return m >= lim;
}
