// gas_switches.h -- the run-time switches a context takes from the environment, read in one place and once per context
// (gas_ctx_create).  Development aids and A/B switches: a product leaves them all unset.  Changing a variable after a
// context exists does not reach that context: its kernel choices, and with GAS_SHELF_SCAN its roundings, stay what they
// were at creation for the whole stream.  No HIP here: plain C++, so that the reader can be tested on its own
// (tests/switches_host_program.cpp).  Not here, by design: GAS_UNI12_MIN / GAS_NT_HIST_MIN (process-wide, with the
// gas_tune_* setters of gas_amd.h) and GAS_MULTI_DIRECT / GAS_MULTI_THREADS (read once when a multi-context is created).
#pragma once
#include <cstdint>
#include <cstdlib>

#define GAS_XCD_ORDER_AUTO_MIN 0xFFFFFFFFu // callbacks of at least this many sources are ordered without the flag: never (measured: no net gain at any size); the environment variable of the same name overrides for experiments

struct gas_switches {
	bool rows_first = false; // GAS_STREAM_ROWS_FIRST: plain [HRTF] stream lists sample rows first too (tools/time_stream_loops.py compares the routes)
	bool adpcm_span = true; // GAS_ADPCM_SPAN: 0 = every load decodes from its checkpoint (k_sample_adpcm.hip; tools/time_stream_adpcm.py and the tests compare the paths)
	bool qoa_span = true; // GAS_QOA_SPAN: 0 = every load decodes from its record (k_sample_qoa.hip; tools/time_stream_qoa.py and the tests compare the paths)
	bool uni_flt = true; // GAS_UNI_FLT: [filter, HRTF] through k_hrtf_uni<FLT> (0: the filter stage and the HRTF stage as two launches, for comparison)
	// GAS_UNI_ER: [ER, HRTF] through k_hrtf_uni<ER>.  1 (default): when at most a quarter of the callback's playbacks want
	// their exact peak.  In throughput mode it is the faster form (the launch carries the previous callback's sum, which
	// k_hrtf_ols<ER> has no registers to park: 20.4 vs 22.4 us for cfg5), an ordered callback is a tie (22.7 / 22.4 us) --
	// the choice does not look at the mode, so the two modes stay bit-identical -- and with every peak exact the split
	// kernel's exact-peak workgroups win (23.6 vs 25.8 us).  0: never.  2: always (tests, A/B).  Staged chains that END in
	// [ER, HRTF] take it whenever it is not 0 (one launch less, no rows in between).
	int uni_er_mode = 1;
	uint32_t xcd_order_auto_min = GAS_XCD_ORDER_AUTO_MIN; // GAS_XCD_ORDER_AUTO_MIN, a decimal source count (experiments)
	bool shelf_scan = true; // GAS_SHELF_SCAN: 0 = rows-out filter stages keep the serial kernel (k_shelf_scan.hip, A/B)
	bool biquad_pipe = true; // GAS_BIQUAD_PIPE: 0 = small callbacks keep the single-wave kernel (k_biquad_pipe.hip, A/B)
};

// One parse per value type; an unset variable leaves the default.
inline bool gas_env_bool(const char *name, bool unset) {
	const char *v = std::getenv(name);
	return v ? std::atoi(v) != 0 : unset;
}
inline int gas_env_int(const char *name, int unset) {
	const char *v = std::getenv(name);
	return v ? std::atoi(v) : unset;
}
inline uint32_t gas_env_u32(const char *name, uint32_t unset) {
	const char *v = std::getenv(name);
	return v ? (uint32_t)std::strtoul(v, nullptr, 10) : unset;
}

inline gas_switches gas_switches_from_env() {
	gas_switches s;
	s.rows_first = gas_env_bool("GAS_STREAM_ROWS_FIRST", s.rows_first);
	s.adpcm_span = gas_env_bool("GAS_ADPCM_SPAN", s.adpcm_span);
	s.qoa_span = gas_env_bool("GAS_QOA_SPAN", s.qoa_span);
	s.uni_flt = gas_env_bool("GAS_UNI_FLT", s.uni_flt);
	s.uni_er_mode = gas_env_int("GAS_UNI_ER", s.uni_er_mode);
	s.xcd_order_auto_min = gas_env_u32("GAS_XCD_ORDER_AUTO_MIN", s.xcd_order_auto_min);
	s.shelf_scan = gas_env_bool("GAS_SHELF_SCAN", s.shelf_scan);
	s.biquad_pipe = gas_env_bool("GAS_BIQUAD_PIPE", s.biquad_pipe);
	return s;
}
