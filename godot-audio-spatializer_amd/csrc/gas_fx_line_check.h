// gas_fx_line_check.h -- the ranges of gas_fx_line_settings (the engine's property ranges), shared by
// gas_fx_line_settings_publish (gas_ctx_fx.hip) and gas_host_set_effect_settings_line (the host layer).  Plain C++, no
// HIP: the host layer is also built for the CPU.  Not part of the ABI.
#pragma once

#include <cmath>

#include "../../include/gas_amd.h"

inline bool gas_in_range(float v, float lo, float hi) { // NaN is out of every range
	return v >= lo && v <= hi;
}

inline bool gas_fx_line_settings_valid(const gas_fx_line_settings &d) {
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		const bool ok = gas_in_range(d.delay_dry[j], 0.0f, 1.0f) && gas_in_range(d.delay_tap1_ms[j], 0.0f, 1500.0f) && gas_in_range(d.delay_tap2_ms[j], 0.0f, 1500.0f) && gas_in_range(d.delay_feedback_ms[j], 0.0f, 1500.0f) && gas_in_range(d.delay_tap1_pan[j], -1.0f, 1.0f) && gas_in_range(d.delay_tap2_pan[j], -1.0f, 1.0f) && std::isfinite(d.delay_tap1_level_db[j]) && std::isfinite(d.delay_tap2_level_db[j]) && std::isfinite(d.delay_feedback_level_db[j]) && gas_in_range(d.delay_feedback_lowpass_hz[j], 1.0f, 16000.0f) && gas_in_range(d.reverb_predelay_ms[j], 20.0f, 500.0f) && gas_in_range(d.reverb_predelay_feedback[j], 0.0f, 0.98f) && gas_in_range(d.reverb_room_size[j], 0.0f, 1.0f) && gas_in_range(d.reverb_damping[j], 0.0f, 1.0f) && gas_in_range(d.reverb_spread[j], 0.0f, 1.0f) && gas_in_range(d.reverb_hipass[j], 0.0f, 1.0f) && gas_in_range(d.reverb_dry[j], 0.0f, 1.0f) && gas_in_range(d.reverb_wet[j], 0.0f, 1.0f);
		if (!ok) {
			return false;
		}
	}
	return true;
}
