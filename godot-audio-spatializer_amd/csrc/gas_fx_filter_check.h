// gas_fx_filter_check.h -- what gas_fx_filter_settings may hold (the engine's enums and property ranges), shared by
// gas_fx_filter_settings_publish (gas_ctx_fx.hip) and gas_host_set_effect_settings_filter (the host layer).  Plain C++,
// no HIP: the host layer is also built for the CPU.  Not part of the ABI.
#pragma once

#include "gas_fx_line_check.h"

inline bool gas_fx_filter_settings_valid(const gas_fx_filter_settings &d) { // every position, used or not
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		const bool ok = d.type[j] >= GAS_FILTER_LOWPASS && d.type[j] <= GAS_FILTER_BANDLIMIT && d.db[j] >= GAS_FILTER_6DB && d.db[j] <= GAS_FILTER_24DB && gas_in_range(d.cutoff_hz[j], 1.0f, 20500.0f) && gas_in_range(d.resonance[j], 0.0f, 1.0f) && gas_in_range(d.gain[j], 0.0f, 4.0f);
		if (!ok) {
			return false;
		}
		// the engine takes log(resonance) for the band limit's bandwidth: NaN coefficients at 0
		if (d.type[j] == GAS_FILTER_BANDLIMIT && !(d.resonance[j] > 0.0f)) {
			return false;
		}
	}
	return true;
}

// [ENGINE] AudioEffectFilter resource defaults (gas_amd.h)
inline gas_fx_filter_settings gas_fx_filter_settings_defaults() {
	gas_fx_filter_settings d{};
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		d.type[j] = GAS_FILTER_LOWPASS;
		d.db[j] = GAS_FILTER_6DB;
		d.cutoff_hz[j] = 2000.0f;
		d.resonance[j] = 0.5f;
		d.gain[j] = 1.0f;
	}
	return d;
}
