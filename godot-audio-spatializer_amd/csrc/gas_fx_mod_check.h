// gas_fx_mod_check.h -- the ranges of gas_fx_mod_settings (the engine's property ranges), shared by
// gas_fx_mod_settings_publish (gas_ctx_fx.hip) and gas_host_set_effect_settings_mod (the host layer).  Plain C++, no HIP:
// the host layer is also built for the CPU.  Not part of the ABI.
#pragma once

#include "gas_fx_line_check.h"

inline bool gas_fx_mod_settings_valid(const gas_fx_mod_settings &d) { // every position and voice, used or not
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		bool ok = d.chorus_voice_count[j] >= 1 && d.chorus_voice_count[j] <= GAS_CHORUS_MAX_VOICES && gas_in_range(d.chorus_dry[j], 0.0f, 1.0f) && gas_in_range(d.chorus_wet[j], 0.0f, 1.0f) && gas_in_range(d.phaser_range_min_hz[j], 10.0f, 10000.0f) && gas_in_range(d.phaser_range_max_hz[j], 10.0f, 10000.0f) && gas_in_range(d.phaser_rate_hz[j], 0.01f, 20.0f) && gas_in_range(d.phaser_feedback[j], 0.1f, 0.9f) && gas_in_range(d.phaser_depth[j], 0.1f, 4.0f);
		for (int v = 0; v < GAS_CHORUS_MAX_VOICES && ok; v++) {
			ok = gas_in_range(d.chorus_delay_ms[j][v], 0.0f, 50.0f) && gas_in_range(d.chorus_rate_hz[j][v], 0.1f, 20.0f) && gas_in_range(d.chorus_depth_ms[j][v], 0.0f, 20.0f) && gas_in_range(d.chorus_level_db[j][v], -60.0f, 24.0f) && gas_in_range(d.chorus_cutoff_hz[j][v], 1.0f, 20500.0f) && gas_in_range(d.chorus_pan[j][v], -1.0f, 1.0f);
		}
		if (!ok) {
			return false;
		}
	}
	return true;
}

// [ENGINE] AudioEffectChorus / AudioEffectPhaser resource defaults (gas_amd.h)
inline gas_fx_mod_settings gas_fx_mod_settings_defaults() {
	static const float delay[4] = { 15.0f, 20.0f, 12.0f, 12.0f }, rate[4] = { 0.8f, 1.2f, 1.0f, 1.0f };
	static const float depth[4] = { 2.0f, 3.0f, 0.0f, 0.0f }, cutoff[4] = { 8000.0f, 8000.0f, 16000.0f, 16000.0f };
	static const float pan[4] = { -0.5f, 0.5f, 0.0f, 0.0f };
	gas_fx_mod_settings d{};
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		d.chorus_voice_count[j] = 2;
		d.chorus_dry[j] = 1.0f;
		d.chorus_wet[j] = 0.5f;
		for (int v = 0; v < GAS_CHORUS_MAX_VOICES; v++) {
			d.chorus_delay_ms[j][v] = delay[v];
			d.chorus_rate_hz[j][v] = rate[v];
			d.chorus_depth_ms[j][v] = depth[v];
			d.chorus_level_db[j][v] = 0.0f;
			d.chorus_cutoff_hz[j][v] = cutoff[v];
			d.chorus_pan[j][v] = pan[v];
		}
		d.phaser_range_min_hz[j] = 440.0f;
		d.phaser_range_max_hz[j] = 1600.0f;
		d.phaser_rate_hz[j] = 0.5f;
		d.phaser_feedback[j] = 0.7f;
		d.phaser_depth[j] = 1.0f;
	}
	return d;
}
