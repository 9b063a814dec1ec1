// gas_fx_eq_check.h -- the range of gas_fx_eq_settings (the engine's band gain range, -60 .. 24 dB), shared by
// gas_fx_eq_settings_publish (gas_ctx_fx.hip) and gas_host_set_effect_settings_eq (the host layer).  Plain C++, no HIP: the
// host layer is also built for the CPU.  Not part of the ABI.
#pragma once

#include "gas_fx_line_check.h"

inline bool gas_fx_eq_settings_valid(const gas_fx_eq_settings &d) { // every position and band, used or not
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		for (int k = 0; k < GAS_EQ_MAX_BANDS; k++) {
			if (!gas_in_range(d.band_gain_db[j][k], -60.0f, 24.0f)) {
				return false;
			}
		}
	}
	return true;
}
