// gas_fx_dyn_check.h -- the rule of gas_fx_dyn_settings (a known distortion mode; compressor ratio, attack and release
// above zero; a compressor sidechain of 0 .. GAS_MAX_SIDECHAINS), shared by gas_fx_dyn_settings_publish (gas_ctx_fx.hip) and gas_host_set_effect_settings_dyn (the host
// layer).  Plain C++, no HIP: the host layer is also built for the CPU.  Not part of the ABI.
#pragma once

#include "../../include/gas_amd.h"

inline bool gas_fx_dyn_settings_valid(const gas_fx_dyn_settings &d) { // every position, used or not; NaN fails
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		if (d.distortion_mode[j] < GAS_DISTORTION_CLIP || d.distortion_mode[j] > GAS_DISTORTION_WAVESHAPE || !(d.compressor_ratio[j] > 0.0f) || !(d.compressor_attack_us[j] > 0.0f) || !(d.compressor_release_ms[j] > 0.0f) || d.compressor_sidechain[j] > GAS_MAX_SIDECHAINS) {
			return false;
		}
	}
	return true;
}
