// gas_fx_stereo_check.h -- the ranges of gas_fx_stereo_settings (the engine's property ranges), shared by
// gas_fx_stereo_settings_publish (gas_ctx_fx.hip) and gas_host_set_effect_settings_stereo (the host layer).  Plain C++,
// no HIP: the host layer is also built for the CPU.  Not part of the ABI.
#pragma once

#include "gas_fx_line_check.h"

inline bool gas_fx_stereo_settings_valid(const gas_fx_stereo_settings &d) { // every position, used or not
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		const bool ok = gas_in_range(d.panner_pan[j], -1.0f, 1.0f) && gas_in_range(d.enhance_pan_pullout[j], 0.0f, 4.0f) && gas_in_range(d.enhance_time_pullout_ms[j], 0.0f, 50.0f) && gas_in_range(d.enhance_surround[j], 0.0f, 1.0f) && gas_in_range(d.limiter_ceiling_db[j], -20.0f, -0.1f) && gas_in_range(d.limiter_threshold_db[j], -30.0f, 0.0f) && gas_in_range(d.limiter_soft_clip_db[j], 0.0f, 6.0f) && gas_in_range(d.limiter_soft_clip_ratio[j], 3.0f, 20.0f);
		if (!ok) {
			return false;
		}
	}
	return true;
}

// [ENGINE] AudioEffectPanner / AudioEffectStereoEnhance / AudioEffectLimiter resource defaults (gas_amd.h)
inline gas_fx_stereo_settings gas_fx_stereo_settings_defaults() {
	gas_fx_stereo_settings d{};
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		d.enhance_pan_pullout[j] = 1.0f;
		d.limiter_ceiling_db[j] = -0.1f;
		d.limiter_soft_clip_db[j] = 2.0f;
		d.limiter_soft_clip_ratio[j] = 10.0f;
	}
	return d;
}
