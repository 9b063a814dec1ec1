// gas_ctx_fx.hip -- the effect families: the table that describes them, their life cycle -- reserve,
// hand out, publish, flush, reset, free, release -- the stage launch of a staged chain, and the
// gas_fx_*_settings_publish / gas_ctx_reserve_fx_* entries of include/gas_amd.h.  The rest of the library reaches the
// families through the few calls declared in gas_ctx_priv.h (the middle of this file); the table is file-local.
#include "gas_ctx_priv.h"

namespace {

// [ENGINE] AudioEffectFilter / AudioEffectAmplify resource defaults
gas_fx_settings fx_settings_defaults() {
	gas_fx_settings d;
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		d.filter_cutoff_hz[j] = 2000.0f;
		d.filter_resonance[j] = 0.5f;
		d.filter_gain[j] = 1.0f;
		d.amplify_volume_db[j] = 0.0f;
	}
	return d;
}

// [ENGINE] AudioEffectDistortion / AudioEffectCompressor resource defaults
gas_fx_dyn_settings fx_dyn_settings_defaults() {
	gas_fx_dyn_settings d;
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		d.distortion_mode[j] = GAS_DISTORTION_CLIP;
		d.distortion_pre_gain_db[j] = 0.0f;
		d.distortion_keep_hf_hz[j] = 16000.0f;
		d.distortion_drive[j] = 0.0f;
		d.distortion_post_gain_db[j] = 0.0f;
		d.compressor_threshold_db[j] = 0.0f;
		d.compressor_ratio[j] = 4.0f;
		d.compressor_gain_db[j] = 0.0f;
		d.compressor_attack_us[j] = 20.0f;
		d.compressor_release_ms[j] = 250.0f;
		d.compressor_mix[j] = 1.0f;
		d.compressor_sidechain[j] = 0;
	}
	return d;
}

// [ENGINE] AudioEffectDelay / AudioEffectReverb resource defaults
gas_fx_line_settings fx_line_settings_defaults() {
	gas_fx_line_settings d;
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		d.delay_dry[j] = 1.0f;
		d.delay_tap1_active[j] = 1;
		d.delay_tap1_ms[j] = 250.0f;
		d.delay_tap1_level_db[j] = -6.0f;
		d.delay_tap1_pan[j] = 0.2f;
		d.delay_tap2_active[j] = 1;
		d.delay_tap2_ms[j] = 500.0f;
		d.delay_tap2_level_db[j] = -12.0f;
		d.delay_tap2_pan[j] = -0.4f;
		d.delay_feedback_active[j] = 0;
		d.delay_feedback_ms[j] = 340.0f;
		d.delay_feedback_level_db[j] = -6.0f;
		d.delay_feedback_lowpass_hz[j] = 16000.0f;
		d.reverb_predelay_ms[j] = 150.0f;
		d.reverb_predelay_feedback[j] = 0.4f;
		d.reverb_room_size[j] = 0.8f;
		d.reverb_damping[j] = 0.5f;
		d.reverb_spread[j] = 1.0f;
		d.reverb_hipass[j] = 0.0f;
		d.reverb_dry[j] = 1.0f;
		d.reverb_wet[j] = 0.5f;
	}
	return d;
}

// Line geometry at a mix rate: the engine's Freeverb tunings in seconds, the two ears' extra spread.
gas_line_geo make_line_geo(float mix_rate) {
	static const double ct[8] = { 0.025306122448979593, 0.026938775510204082, 0.028956916099773241, 0.03074829931972789, 0.032244897959183672, 0.03380952380952381, 0.035306122448979592, 0.036666666666666667 };
	static const double at[4] = { 0.0051020408163265302, 0.007732426303854875, 0.01, 0.012607709750566893 };
	static const double spread_base[2] = { 0.0, 0.000521 };
	const double sr = (double)mix_rate;
	gas_line_geo g{};
	const uint32_t fb = (uint32_t)(int)(1.5 * sr) + 1;
	uint32_t ring = 1;
	while (ring < fb + 512) { // longer than the longest tap by more than a block (k_fx_line.hip)
		ring *= 2;
	}
	g.ring_mask = ring - 1;
	g.fb_frames = fb;
	g.delay_floats = ((GAS_LINE_HEADER + 2 * (size_t)ring + 2 * (size_t)fb) + 63) / 64 * 64;
	g.echo_size = (uint32_t)(int)(0.5 * sr + 1.0);
	size_t off = GAS_LINE_HEADER;
	for (int e = 0; e < 2; e++) {
		g.xs[e] = (uint32_t)lrint(spread_base[e] * sr);
		g.echo_off[e] = (uint32_t)off;
		off += g.echo_size;
		for (int k = 0; k < 8; k++) {
			g.comb_size[e][k] = (uint32_t)lrint(ct[k] * sr) + g.xs[e];
			g.comb_off[e][k] = (uint32_t)off;
			off += g.comb_size[e][k];
		}
		for (int k = 0; k < 4; k++) {
			g.ap_size[e][k] = (uint32_t)lrint(at[k] * sr) + g.xs[e];
			g.ap_off[e][k] = (uint32_t)off;
			off += g.ap_size[e][k];
		}
	}
	for (int k = 0; k < 4; k++) {
		g.ap_base[k] = (uint32_t)lrint(at[k] * sr);
	}
	g.reverb_floats = (off + 63) / 64 * 64;
	return g;
}

constexpr int line_pool_of(int kind) { // 0 delay, 1 reverb, -1 no line
	return kind == GAS_FX_DELAY ? 0 : (kind == GAS_FX_REVERB ? 1 : -1);
}

// [ENGINE] the EQ6 / EQ10 / EQ21 presets' band centres (Hz)
const double k_eq_freqs6[6] = { 32, 100, 320, 1000, 3200, 10000 };
const double k_eq_freqs10[10] = { 31.25, 62.5, 125, 250, 500, 1000, 2000, 4000, 8000, 16000 };
const double k_eq_freqs21[21] = { 22, 32, 44, 63, 90, 125, 175, 250, 350, 500, 700, 1000, 1400, 2000, 2800, 4000, 5600, 8000, 11000, 16000, 22000 };

// [ENGINE] EQ::recalculate_band_coefficients in f64, rounded to f32.  A band whose formula has no real
// root (a == 0 or a negative discriminant: the engine skips it and leaves its coefficients unset) gets c1 = c2 = c3 = 0.
gas_eq_coefs make_eq_coefs(int kind, float mix_rate) {
	const int B = gas_eq_bands(kind);
	const double *f = kind == GAS_FX_EQ6 ? k_eq_freqs6 : (kind == GAS_FX_EQ10 ? k_eq_freqs10 : k_eq_freqs21);
	const double sr = (double)mix_rate;
	gas_eq_coefs q{};
	for (int i = 0; i < B; i++) {
		double octave_size;
		if (i == 0) {
			octave_size = log2(f[1]) - log2(f[0]);
		} else if (i == B - 1) {
			octave_size = log2(f[i]) - log2(f[i - 1]);
		} else {
			octave_size = ((log2(f[i]) - log2(f[i - 1])) + (log2(f[i + 1]) - log2(f[i]))) * 0.5;
		}
		const double frq_l = round(f[i] / pow(2.0, octave_size / 2.0));
		const double s = 0.5; // sqrt(1/2) squared
		const double th = 2.0 * M_PI * f[i] / sr, th_l = 2.0 * M_PI * frq_l / sr;
		const double ct = cos(th), ctl = cos(th_l), stl = sin(th_l);
		const double a = s * ct * ct - 2.0 * s * ctl * ct + s - stl * stl;
		const double b = 2.0 * s * ctl * ctl + s * ct * ct - 2.0 * s * ctl * ct - s + stl * stl;
		const double c = 0.25 * s * ct * ct - 0.5 * s * ctl * ct + 0.25 * s - 0.25 * stl * stl;
		const double disc = b * b - 4.0 * a * c;
		if (a == 0.0 || disc < 0.0) {
			continue;
		}
		const double r1 = (-b + sqrt(disc)) / (2.0 * a);
		q.c1[i] = (float)(2.0 * (0.5 - r1) / 2.0);
		q.c2[i] = (float)(2.0 * r1);
		q.c3[i] = (float)(2.0 * (0.5 + r1) * ct);
	}
	return q;
}

constexpr bool is_eq(int kind) {
	return kind >= GAS_FX_EQ6 && kind <= GAS_FX_EQ21;
}

gas_fx_eq_settings fx_eq_settings_defaults() {
	return gas_fx_eq_settings{}; // 0 dB everywhere
}

constexpr int mod_pool_of(int kind) { // 0 chorus line, 1 phaser bank, -1 neither
	return kind == GAS_FX_CHORUS ? 0 : (kind == GAS_FX_PHASER ? 1 : -1);
}

constexpr bool is_stereo(int kind) { // k_fx_stereo.hip's kinds
	return kind >= GAS_FX_PANNER && kind <= GAS_FX_LIMITER;
}

// ---------------------------------------------------------------------------------------------------------------
// The effect families: one life cycle -- reserve, hand out, publish, flush, reset, free, release --
// and one stage launch over a description of what differs between them.
// ---------------------------------------------------------------------------------------------------------------

// A family's members of gas_dev_state.
struct FxDev {
	void *settings = nullptr; // [max_sources] settings PODs, by chain position
	int32_t *of = nullptr; // [GAS_MAX_EFFECTS][max_sources] pool entry of chain position j, -1: none (nullptr: a family without pools)
	float *pool[2] = { nullptr, nullptr };
};

template <class S, S *gas_dev_state::*Settings, int32_t *gas_dev_state::*Of = nullptr, float *gas_dev_state::*Pool0 = nullptr, float *gas_dev_state::*Pool1 = nullptr>
struct FxDevOf {
	static FxDev get(const gas_dev_state &st) {
		FxDev d;
		d.settings = st.*Settings;
		if constexpr (Of != nullptr) {
			d.of = st.*Of;
		}
		if constexpr (Pool0 != nullptr) {
			d.pool[0] = st.*Pool0;
		}
		if constexpr (Pool1 != nullptr) {
			d.pool[1] = st.*Pool1;
		}
		return d;
	}
	static void set(gas_dev_state &st, const FxDev &d) {
		st.*Settings = static_cast<S *>(d.settings);
		if constexpr (Of != nullptr) {
			st.*Of = d.of;
		}
		if constexpr (Pool0 != nullptr) {
			st.*Pool0 = d.pool[0];
		}
		if constexpr (Pool1 != nullptr) {
			st.*Pool1 = d.pool[1];
		}
	}
};
using BasicDev = FxDevOf<gas_fx_settings, &gas_dev_state::fxs>;
using DynDev = FxDevOf<gas_fx_dyn_settings, &gas_dev_state::dyn>;
using LinesDev = FxDevOf<gas_fx_line_settings, &gas_dev_state::line_settings, &gas_dev_state::line_of, &gas_dev_state::delay_pool, &gas_dev_state::reverb_pool>;
using EqDev = FxDevOf<gas_fx_eq_settings, &gas_dev_state::eq_settings, &gas_dev_state::eq_of, &gas_dev_state::eq_pool>;
using FilterDev = FxDevOf<gas_fx_filter_settings, &gas_dev_state::flt_settings, &gas_dev_state::flt_of, &gas_dev_state::flt_pool>;
using ModDev = FxDevOf<gas_fx_mod_settings, &gas_dev_state::mod_settings, &gas_dev_state::mod_of, &gas_dev_state::chorus_pool, &gas_dev_state::phaser_pool>;
using StereoDev = FxDevOf<gas_fx_stereo_settings, &gas_dev_state::stereo_settings, &gas_dev_state::stereo_of, &gas_dev_state::enhance_pool>;

template <class S, S (*Defaults)()>
void fx_defaults_of(void *row) {
	*static_cast<S *>(row) = Defaults();
}

template <class S, bool (*Valid)(const S &)>
bool fx_valid_of(const void *row) {
	return Valid(*static_cast<const S *>(row));
}

struct FxFamilyDesc {
	const char *name; // gas_ctx_reserve_fx_<name>, for its error strings
	uint32_t pod_bytes; // the settings POD
	void (*defaults)(void *row); // the engine's resource defaults
	bool (*valid)(const void *row); // gas_fx_*_check.h (nullptr: every row is taken)
	int (*pool_of)(int kind); // the pool an effect kind takes its entry from, -1: none
	bool (*has_kind)(int kind); // the kinds whose settings the POD carries: no kind is in two families (k_fx_kinds)
	bool resident; // settings, table and staging buffer exist from gas_ctx_create on, a reservation adds the pool
	FxDev (*get)(const gas_dev_state &st);
	void (*set)(gas_dev_state &st, const FxDev &d);
	int (*check)(const gas_ctx *c, const uint32_t *counts); // what a reservation asks of the context (nullptr: nothing)
	size_t (*entry_floats)(const gas_ctx *c, int pool); // nullptr: a family without pools (no reservation, no slot -> entry table on the device)
	void (*extras)(gas_ctx *c, bool reserved); // what the kernels need besides the pools: set by a reservation, dropped by a release (nullptr: nothing)
	hipError_t (*launch)(const gas_ctx *c, int kind, const gas_group_args &in, uint32_t chain_pos, gas_audio_frame *rows_out); // a stage of a staged chain
};

// [ENGINE] AudioEffectChorus's ring: 1 << bitlength((int)(0.24 sr)) frames; AudioEffectStereoEnhance's: of
// (int)((50 + 2) / 1000 sr)
uint32_t ring_frames(uint32_t n) {
	uint32_t bits = 0;
	while (bits < 31 && (n >> bits) != 0) {
		bits++;
	}
	return 1u << bits;
}

uint32_t chorus_ring_frames(const gas_ctx *c) {
	return ring_frames((uint32_t)(int)(0.24 * (double)c->cfg.mix_rate));
}

uint32_t enhance_ring_frames(const gas_ctx *c) {
	return ring_frames((uint32_t)(int)((50.0 + 2.0) / 1000.0 * (double)c->cfg.mix_rate));
}

int lines_check(const gas_ctx *c, const uint32_t *counts) {
	const double sr = (double)c->cfg.mix_rate;
	const long F = (long)c->cfg.frames;
	// the reverb kernel's predelay and comb reads must not reach the block's own writes
	return counts[1] > 0 && (lrint(0.02 * sr) < F || lrint(0.025306122 * sr) < F) ? GAS_ERR_INVALID_ARGUMENT : GAS_OK;
}

int mod_check(const gas_ctx *c, const uint32_t *counts) {
	const double sr = (double)c->cfg.mix_rate;
	// one block's ring writes must not overtake its own oldest read
	return counts[0] > 0 && (long)chorus_ring_frames(c) < lrint(0.05 * sr) + 2L * (int)(0.02 * sr) + 12 + (long)c->cfg.frames ? GAS_ERR_INVALID_ARGUMENT : GAS_OK;
}

int stereo_check(const gas_ctx *c, const uint32_t *counts) {
	const uint32_t R = enhance_ring_frames(c);
	return counts[0] > 0 && (R < c->cfg.frames || R < 4) ? GAS_ERR_INVALID_ARGUMENT : GAS_OK; // two frames of one block would share a ring entry
}

constexpr int no_pool(int) {
	return -1;
}

constexpr FxFamilyDesc k_fx_families[FX_FAMILIES] = {
	// the engine's other one-biquad filters and the amplifier: k_biquad_mix's rows-out form (its partial-mix arguments
	// are not read then), state in the slot's processor stream of chain position j
	{ "basic", sizeof(gas_fx_settings), fx_defaults_of<gas_fx_settings, fx_settings_defaults>, nullptr, no_pool,
			[](int kind) { return kind >= GAS_FX_LOWPASS && kind <= GAS_FX_AMPLIFY; }, true, BasicDev::get, BasicDev::set, nullptr, nullptr, nullptr,
			[](const gas_ctx *c, int kind, const gas_group_args &in, uint32_t j, gas_audio_frame *out) {
				gas_biquad_launch lb = biquad_launch(c, kind == GAS_FX_AMPLIFY ? GAS_MODE_FX_AMPLIFY : GAS_MODE_FX_FILTER, in, c->d_partials, 0);
				lb.channel_begin = j;
				lb.rows_out = reinterpret_cast<float *>(out);
				lb.fx_kind = kind;
				return gas_launch_biquad_mix(lb);
			} },
	{ "dyn", sizeof(gas_fx_dyn_settings), fx_defaults_of<gas_fx_dyn_settings, fx_dyn_settings_defaults>, fx_valid_of<gas_fx_dyn_settings, gas_fx_dyn_settings_valid>, no_pool,
			[](int kind) { return kind == GAS_FX_DISTORTION || kind == GAS_FX_COMPRESSOR; }, true, DynDev::get, DynDev::set, nullptr, nullptr, nullptr,
			[](const gas_ctx *c, int kind, const gas_group_args &in, uint32_t j, gas_audio_frame *out) { return gas_launch_fx_dyn(c->stream, kind, in, c->st, c->cfg.frames, j, c->cfg.mix_rate, out); } },
	{ "lines", sizeof(gas_fx_line_settings), fx_defaults_of<gas_fx_line_settings, fx_line_settings_defaults>, fx_valid_of<gas_fx_line_settings, gas_fx_line_settings_valid>, line_pool_of,
			[](int kind) { return line_pool_of(kind) >= 0; }, false, LinesDev::get, LinesDev::set, lines_check,
			[](const gas_ctx *c, int pool) { const gas_line_geo g = make_line_geo(c->cfg.mix_rate); return pool == 0 ? g.delay_floats : g.reverb_floats; },
			[](gas_ctx *c, bool reserved) {
				if (reserved) {
					c->line_geo = make_line_geo(c->cfg.mix_rate);
				}
			},
			[](const gas_ctx *c, int kind, const gas_group_args &in, uint32_t j, gas_audio_frame *out) { return gas_launch_fx_line(c->stream, kind, in, c->st, c->line_geo, c->cfg.frames, j, c->cfg.mix_rate, out); } },
	{ "eq", sizeof(gas_fx_eq_settings), fx_defaults_of<gas_fx_eq_settings, fx_eq_settings_defaults>, fx_valid_of<gas_fx_eq_settings, gas_fx_eq_settings_valid>,
			[](int kind) { return is_eq(kind) ? 0 : -1; }, is_eq, false, EqDev::get, EqDev::set, nullptr,
			[](const gas_ctx *, int) { return (size_t)GAS_EQ_BANK_FLOATS; },
			[](gas_ctx *c, bool reserved) {
				for (int k = 0; k < 3 && reserved; k++) {
					c->eq_coefs[k] = make_eq_coefs(GAS_FX_EQ6 + k, c->cfg.mix_rate);
				}
			},
			[](const gas_ctx *c, int kind, const gas_group_args &in, uint32_t j, gas_audio_frame *out) { return gas_launch_fx_eq(c->stream, kind, in, c->st, c->eq_coefs[kind - GAS_FX_EQ6], c->cfg.frames, j, out); } },
	{ "filter", sizeof(gas_fx_filter_settings), fx_defaults_of<gas_fx_filter_settings, gas_fx_filter_settings_defaults>, fx_valid_of<gas_fx_filter_settings, gas_fx_filter_settings_valid>,
			[](int kind) { return kind == GAS_FX_FILTER ? 0 : -1; }, [](int kind) { return kind == GAS_FX_FILTER; }, false, FilterDev::get, FilterDev::set, nullptr,
			[](const gas_ctx *, int) { return (size_t)GAS_FILTER_BANK_FLOATS; }, nullptr,
			[](const gas_ctx *c, int, const gas_group_args &in, uint32_t j, gas_audio_frame *out) { return gas_launch_fx_filter(c->stream, in, c->st, c->cfg.frames, j, c->cfg.mix_rate, out); } },
	{ "mod", sizeof(gas_fx_mod_settings), fx_defaults_of<gas_fx_mod_settings, gas_fx_mod_settings_defaults>, fx_valid_of<gas_fx_mod_settings, gas_fx_mod_settings_valid>, mod_pool_of,
			[](int kind) { return mod_pool_of(kind) >= 0; }, false, ModDev::get, ModDev::set, mod_check,
			[](const gas_ctx *c, int pool) { return pool == 0 ? GAS_CHORUS_HEADER + 2 * (size_t)chorus_ring_frames(c) : (size_t)GAS_PHASER_BANK_FLOATS; },
			[](gas_ctx *c, bool reserved) { c->st.chorus_mask = reserved ? chorus_ring_frames(c) - 1 : 0; },
			[](const gas_ctx *c, int kind, const gas_group_args &in, uint32_t j, gas_audio_frame *out) { return gas_launch_fx_mod(c->stream, kind, in, c->st, c->cfg.frames, j, c->cfg.mix_rate, out); } },
	// panner and limiter need no reservation: only the stereo enhance takes a ring
	{ "stereo", sizeof(gas_fx_stereo_settings), fx_defaults_of<gas_fx_stereo_settings, gas_fx_stereo_settings_defaults>, fx_valid_of<gas_fx_stereo_settings, gas_fx_stereo_settings_valid>,
			[](int kind) { return kind == GAS_FX_STEREO_ENHANCE ? 0 : -1; }, is_stereo, true, StereoDev::get, StereoDev::set, stereo_check,
			[](const gas_ctx *c, int) { return GAS_ENHANCE_HEADER + (size_t)enhance_ring_frames(c); },
			[](gas_ctx *c, bool reserved) { c->st.enhance_mask = reserved ? enhance_ring_frames(c) - 1 : 0; },
			[](const gas_ctx *c, int kind, const gas_group_args &in, uint32_t j, gas_audio_frame *out) { return gas_launch_fx_stereo(c->stream, kind, in, c->st, c->cfg.frames, j, c->cfg.mix_rate, out); } },
};

// kind -> family, filled once from has_kind, so that neither group_of nor a callback's stage loop walks the table
struct FxKinds {
	int8_t family[256];
	bool unique;
};

constexpr FxKinds fx_kinds() {
	FxKinds m{};
	m.unique = true;
	for (int kind = 0; kind < 256; kind++) {
		m.family[kind] = -1;
		for (int f = 0; f < FX_FAMILIES; f++) {
			if (k_fx_families[f].has_kind(kind)) {
				m.unique = m.unique && m.family[kind] < 0;
				m.family[kind] = (int8_t)f;
			}
		}
	}
	return m;
}

constexpr FxKinds k_fx_kinds = fx_kinds();
static_assert(k_fx_kinds.unique, "an effect kind belongs to at most one family");

std::array<int32_t, GAS_MAX_EFFECTS> fx_no_entries() {
	std::array<int32_t, GAS_MAX_EFFECTS> none;
	none.fill(-1);
	return none;
}

// Queues the zeroing of slot s's pool entries (chain signature sig), each entry at most once until the next flush, so
// the queue never holds more records than the pools have entries (the upload buffer's zero section); params_mu held.
void fx_queue_zero(gas_ctx *c, int f, uint32_t s, uint32_t sig) {
	FxFamily &p = c->fx[f];
	const FxFamilyDesc &d = k_fx_families[f];
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		const int kind = (sig >> (8 * j)) & 0xff;
		const int pool = d.pool_of(kind);
		const int32_t idx = p.h_of[s][j];
		if (pool >= 0 && idx >= 0 && !p.zero_pending[pool][idx]) {
			p.zero_pending[pool][idx] = 1;
			p.zero_list.push_back((uint32_t)pool);
			p.zero_list.push_back((uint32_t)idx);
		}
	}
}

// A new slot's entries, one per effect of its chain that takes one, and its settings at the resource defaults: entered
// in the tables and zeroed at the next flush.  alloc_mu held, the entries are there (gas_source_alloc).
void fx_hand_out(gas_ctx *c, int f, uint32_t s, const int32_t *effects, uint32_t n_effects, uint32_t sig) {
	FxFamily &p = c->fx[f];
	const FxFamilyDesc &d = k_fx_families[f];
	std::lock_guard<std::mutex> lk(c->params_mu);
	for (uint32_t j = 0; j < GAS_MAX_EFFECTS; j++) {
		const int pool = j < n_effects ? d.pool_of(effects[j]) : -1;
		if (pool >= 0) {
			p.h_of[s][j] = (int32_t)p.free[pool].back();
			p.free[pool].pop_back();
		} else {
			p.h_of[s][j] = -1;
		}
	}
	d.defaults(p.h_settings.data() + (size_t)s * d.pod_bytes);
	mark_dirty(p.dirty_flag, p.dirty_list, s);
	fx_queue_zero(c, f, s, sig);
}

// A freed slot's entries go back to the pools (zeroed when they are handed out again); alloc_mu held.
void fx_return_entries(gas_ctx *c, int f, uint32_t s, uint32_t sig) {
	FxFamily &p = c->fx[f];
	if (p.cap[0] + p.cap[1] == 0) {
		return;
	}
	std::lock_guard<std::mutex> lk(c->params_mu); // (h_of is read by the flush under params_mu)
	for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
		const int pool = k_fx_families[f].pool_of((sig >> (8 * j)) & 0xff);
		if (pool >= 0 && p.h_of[s][j] >= 0) {
			p.free[pool].push_back((uint32_t)p.h_of[s][j]);
			p.h_of[s][j] = -1;
		}
	}
}

// The staging buffer of fx_flush with room for `entries` zero records; main thread, stream idle.
hipError_t fx_alloc_upload(gas_ctx *c, int f, size_t entries) {
	FxFamily &p = c->fx[f];
	const FxFamilyDesc &d = k_fx_families[f];
	// [<= N settings rows][<= N {slot, entry[4]}][<= every entry once] (mark_dirty / fx_queue_zero)
	const size_t bytes = (size_t)c->cfg.max_sources * (d.pod_bytes + (1 + GAS_MAX_EFFECTS) * sizeof(uint32_t)) + entries * 2 * sizeof(uint32_t);
	size_t cap[2] = { 0, 0 }; // no capacity is kept: the buffers are as large as this reservation needs, never larger
	const hipError_t e = c->mem.grow(p.d_upload, cap[0], bytes);
	const hipError_t eh = c->mem.grow(p.h_upload, cap[1], bytes, 1, Mem::PINNED);
	return e != hipSuccess ? e : eh;
}

// The settings table at the resource defaults (`rows`: the same for the host mirror) and, for a family with pools, the
// slot -> entry table at -1.
hipError_t fx_alloc_tables(gas_ctx *c, int f, FxDev &dev, std::vector<unsigned char> &rows) {
	const FxFamilyDesc &d = k_fx_families[f];
	const size_t N = c->cfg.max_sources, pod = d.pod_bytes;
	rows.resize(N * pod);
	d.defaults(rows.data());
	for (size_t s = 1; s < N; s++) {
		std::memcpy(rows.data() + s * pod, rows.data(), pod);
	}
	hipError_t e = hipSuccess;
	if (d.entry_floats) {
		e = c->mem.alloc(dev.of, GAS_MAX_EFFECTS * N);
		e = e != hipSuccess ? e : hipMemsetAsync(dev.of, 0xff, sizeof(int32_t) * GAS_MAX_EFFECTS * N, c->stream);
	}
	e = e != hipSuccess ? e : c->mem.alloc(dev.settings, N * pod);
	return e != hipSuccess ? e : hipMemcpy(dev.settings, rows.data(), N * pod, hipMemcpyHostToDevice);
}

// Frees the pools and, unless the family is resident, the settings, the table and the staging buffer; params_mu held.
void fx_release(gas_ctx *c, int f) {
	FxFamily &p = c->fx[f];
	const FxFamilyDesc &d = k_fx_families[f];
	FxDev dev = d.get(c->st);
	for (int pl = 0; pl < 2; pl++) {
		c->mem.drop(dev.pool[pl]);
		p.cap[pl] = 0;
		p.free[pl].clear();
		p.zero_pending[pl].clear();
	}
	p.zero_list.clear();
	if (!d.resident) {
		c->mem.drop(dev.of);
		c->mem.drop(dev.settings);
		c->mem.drop(p.d_upload);
		c->mem.drop(p.h_upload);
		p.h_of.clear();
		p.h_settings.clear();
		p.dirty_flag.clear();
		p.dirty_list.clear();
	}
	d.set(c->st, dev);
	if (d.extras) {
		d.extras(c, false);
	}
}

// gas_fx_*_settings_publish: latest wins in the host mirror, uploaded by the next flush.
int fx_publish(gas_ctx *c, int f, const uint32_t *slots, const void *settings, uint32_t n) {
	if (!c || (n > 0 && (!slots || !settings))) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	FxFamily &p = c->fx[f];
	const FxFamilyDesc &d = k_fx_families[f];
	const size_t pod = d.pod_bytes;
	const unsigned char *rows = static_cast<const unsigned char *>(settings);
	for (uint32_t i = 0; i < n; i++) {
		if (slots[i] >= c->cfg.max_sources || !c->slots[slots[i]].used) {
			return GAS_ERR_BAD_SLOT;
		}
		if (d.valid && !d.valid(rows + (size_t)i * pod)) {
			return GAS_ERR_INVALID_ARGUMENT;
		}
	}
	std::lock_guard<std::mutex> lk(c->params_mu);
	if (p.h_settings.empty()) { // nothing reserved: no slot has an effect the settings could reach (never so for a resident family)
		return GAS_OK;
	}
	for (uint32_t i = 0; i < n; i++) {
		std::memcpy(p.h_settings.data() + (size_t)slots[i] * pod, rows + (size_t)i * pod, pod);
		mark_dirty(p.dirty_flag, p.dirty_list, slots[i]);
	}
	return GAS_OK;
}

// The host mirrors that go with fx_alloc_tables' tables: no entries, `rows` as the settings, nothing dirty.
void fx_adopt_tables(gas_ctx *c, int f, std::vector<unsigned char> &rows) {
	FxFamily &p = c->fx[f];
	p.h_of.assign(c->cfg.max_sources, fx_no_entries());
	p.h_settings = std::move(rows);
	p.dirty_flag.assign(c->cfg.max_sources, 0);
}

// gas_ctx_reserve_fx_*: main thread, refused while any entry is held; counts of 0 release everything (a resident
// family keeps its settings, table and a staging buffer without a zero section).
int fx_reserve(gas_ctx *c, int f, uint32_t count0, uint32_t count1) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	FxFamily &p = c->fx[f];
	const FxFamilyDesc &d = k_fx_families[f];
	const uint32_t counts[2] = { count0, count1 };
	const size_t total = (size_t)count0 + count1;
	const int rc = d.check ? d.check(c, counts) : GAS_OK;
	if (rc != GAS_OK) {
		return rc;
	}
	for (int pl = 0; pl < 2; pl++) { // k_zero_entries writes float4: hipMalloc's base and every entry behind it 16-byte aligned
		if (counts[pl] > 0 && d.entry_floats(c, pl) % 4 != 0) {
			return GAS_ERR_INVALID_ARGUMENT; // (no mix rate the checks above accept gets here)
		}
	}
	std::lock_guard<std::mutex> alloc_lk(c->alloc_mu);
	for (int pl = 0; pl < 2; pl++) {
		if (p.free[pl].size() != p.cap[pl]) {
			return GAS_ERR_INVALID_ARGUMENT; // entries are held
		}
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	{
		std::lock_guard<std::mutex> lk(c->params_mu);
		fx_release(c, f);
	}
	if (total == 0 && !d.resident) {
		return GAS_OK;
	}
	std::vector<unsigned char> defaults;
	FxDev dev = d.get(c->st);
	hipError_t e = hipSuccess;
	auto step = [&e](hipError_t r) {
		if (e == hipSuccess) {
			e = r;
		}
	};
	{
		// (queued settings rows live in the mirror only: fx_flush fills the staging buffer per flush)
		std::lock_guard<std::mutex> lk(c->params_mu);
		step(fx_alloc_upload(c, f, total));
	}
	for (int pl = 0; pl < 2; pl++) {
		if (counts[pl]) {
			step(e == hipSuccess ? device_zeroed(c, dev.pool[pl], d.entry_floats(c, pl) * counts[pl]) : e);
		}
	}
	if (!d.resident) {
		step(fx_alloc_tables(c, f, dev, defaults));
	}
	if (total > 0) {
		step(e == hipSuccess ? hipStreamSynchronize(c->stream) : e);
	}
	d.set(c->st, dev);
	if (e != hipSuccess) {
		c->last_err = std::string("gas_ctx_reserve_fx_") + d.name + ": " + hipGetErrorString(e);
		std::lock_guard<std::mutex> lk(c->params_mu);
		fx_release(c, f);
		if (d.resident && (!p.h_upload || !p.d_upload)) {
			(void)fx_alloc_upload(c, f, 0);
		}
		return e == hipErrorOutOfMemory ? GAS_ERR_OUT_OF_MEMORY : GAS_ERR_DEVICE;
	}
	if (total == 0) {
		return GAS_OK;
	}
	std::lock_guard<std::mutex> lk(c->params_mu);
	if (d.extras) {
		d.extras(c, true);
	}
	for (int pl = 0; pl < 2; pl++) { // handed out from entry 0 up
		const uint32_t n = counts[pl];
		p.cap[pl] = n;
		p.zero_pending[pl].assign(n, 0);
		p.free[pl].resize(n);
		for (uint32_t i = 0; i < n; i++) {
			p.free[pl][i] = n - 1 - i;
		}
	}
	if (!d.resident) {
		fx_adopt_tables(c, f, defaults);
	}
	return GAS_OK;
}

} // namespace

namespace gas_priv __attribute__((visibility("hidden"))) {

// Which family carries an effect kind's settings (-1: none).
int family_of(int kind) {
	return kind >= 0 && kind < 256 ? k_fx_kinds.family[kind] : -1;
}

// The stage of a staged chain that runs the kind.
hipError_t fx_launch(const gas_ctx *c, int kind, const gas_group_args &in, uint32_t chain_pos, gas_audio_frame *rows_out) {
	const int f = family_of(kind);
	return f < 0 ? hipErrorInvalidValue : k_fx_families[f].launch(c, kind, in, chain_pos, rows_out);
}

// gas_ctx_create: the families that need no reservation for their settings get table, staging buffer and mirrors here
// (fx_reserve's steps, without pools): every slot starts from the engine's resource defaults.
int fx_create(gas_ctx *c) {
	for (int f = 0; f < FX_FAMILIES; f++) {
		if (k_fx_families[f].resident) {
			FxDev dev;
			std::vector<unsigned char> rows;
			const hipError_t e = fx_alloc_tables(c, f, dev, rows);
			k_fx_families[f].set(c->st, dev);
			GAS_HIP(c, e);
			GAS_HIP(c, fx_alloc_upload(c, f, 0));
			fx_adopt_tables(c, f, rows);
		}
	}
	return GAS_OK;
}

// gas_source_alloc, alloc_mu held: is there room for a chain's pool entries?  GAS_ERR_UNSUPPORTED_CHAIN when a family the
// chain takes entries from has no pool (gas_ctx_reserve_fx_*), GAS_ERR_OUT_OF_SLOTS when a pool has too few free.  Takes
// nothing: the caller checks its slot list too, then fx_slot_new hands out -- all or nothing.
int fx_room(const gas_ctx *c, const int32_t *effects, uint32_t n_effects) {
	bool room = true;
	for (int f = 0; f < FX_FAMILIES; f++) {
		const FxFamily &p = c->fx[f];
		uint32_t need[2] = { 0, 0 }; // pool entries of the chain, per pool
		for (uint32_t j = 0; j < n_effects; j++) {
			const int pool = k_fx_families[f].pool_of(effects[j]);
			if (pool >= 0) {
				need[pool]++;
			}
		}
		if (need[0] + need[1] > 0 && p.cap[0] == 0 && p.cap[1] == 0) {
			return GAS_ERR_UNSUPPORTED_CHAIN;
		}
		room = room && p.free[0].size() >= need[0] && p.free[1].size() >= need[1];
	}
	return room ? GAS_OK : GAS_ERR_OUT_OF_SLOTS;
}

// gas_source_alloc, alloc_mu held, fx_room passed: slot s's entries and defaults in every family the chain has a kind
// of -- a new playback's effect instances start from the resource defaults (audio_spatializer_effect.cpp:79-88).
void fx_slot_new(gas_ctx *c, uint32_t s, const int32_t *effects, uint32_t n_effects, uint32_t sig) {
	for (int f = 0; f < FX_FAMILIES; f++) {
		bool in_family = false;
		for (uint32_t j = 0; j < n_effects; j++) {
			in_family = in_family || k_fx_families[f].has_kind(effects[j]);
		}
		if (in_family) {
			fx_hand_out(c, f, s, effects, n_effects, sig);
		}
	}
}

// apply_pending_frees, alloc_mu held: the freed slot's entries go back to every family's pools.
void fx_slot_freed(gas_ctx *c, uint32_t s, uint32_t sig) {
	for (int f = 0; f < FX_FAMILIES; f++) {
		fx_return_entries(c, f, s, sig);
	}
}

// gas_source_reset: the slot's pool entries are zeroed by the next flush, before the next block (alloc_mu: the audio
// thread may be returning a freed slot's entries; the same lock order as gas_source_alloc).
void fx_slot_reset(gas_ctx *c, uint32_t slot) {
	std::lock_guard<std::mutex> alloc_lk(c->alloc_mu);
	for (int f = 0; f < FX_FAMILIES; f++) {
		if (c->fx[f].cap[0] + c->fx[f].cap[1] > 0 && c->slots[slot].used) {
			std::lock_guard<std::mutex> lk(c->params_mu);
			fx_queue_zero(c, f, slot, c->slots[slot].chain_sig);
		}
	}
}

// What a flush uploads: one copy of [m settings][m {slot, entry[4]}][z {pool, entry} zero records], one scatter, one
// zeroing launch.
int fx_flush(gas_ctx *c, int f) {
	FxFamily &p = c->fx[f];
	const FxFamilyDesc &d = k_fx_families[f];
	if (!d.resident && !p.h_upload) {
		return GAS_OK;
	}
	const size_t pod = d.pod_bytes;
	uint32_t m = 0, z = 0;
	{
		std::lock_guard<std::mutex> lk(c->params_mu);
		m = (uint32_t)p.dirty_list.size();
		z = (uint32_t)p.zero_list.size() / 2;
		if (m == 0 && z == 0) {
			return GAS_OK;
		}
		if (!p.h_upload || !p.d_upload) { // a resident family's failed reservation could not restore it
			return GAS_ERR_OUT_OF_MEMORY;
		}
		uint32_t *hsi = reinterpret_cast<uint32_t *>(p.h_upload + (size_t)m * pod);
		for (uint32_t i = 0; i < m; i++) {
			const uint32_t s = p.dirty_list[i];
			std::memcpy(p.h_upload + (size_t)i * pod, p.h_settings.data() + (size_t)s * pod, pod);
			hsi[i * (1 + GAS_MAX_EFFECTS)] = s;
			for (int j = 0; j < GAS_MAX_EFFECTS; j++) {
				hsi[i * (1 + GAS_MAX_EFFECTS) + 1 + j] = (uint32_t)p.h_of[s][j];
			}
			p.dirty_flag[s] = 0;
		}
		std::memcpy(hsi + (size_t)m * (1 + GAS_MAX_EFFECTS), p.zero_list.data(), (size_t)z * 2 * sizeof(uint32_t));
		for (uint32_t i = 0; i < z; i++) {
			p.zero_pending[p.zero_list[2 * i]][p.zero_list[2 * i + 1]] = 0;
		}
		p.dirty_list.clear();
		p.zero_list.clear();
	}
	const size_t zoff = (size_t)m * (pod + (1 + GAS_MAX_EFFECTS) * sizeof(uint32_t));
	const FxDev dev = d.get(c->st);
	GAS_HIP(c, hipMemcpyAsync(p.d_upload, p.h_upload, zoff + (size_t)z * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	GAS_HIP(c, gas_launch_scatter_fx(c->stream, dev.settings, dev.of, c->st.dyn_stride, d.pod_bytes, p.d_upload, reinterpret_cast<const uint32_t *>(p.d_upload + (size_t)m * pod), m));
	if (z > 0) {
		const size_t floats[2] = { d.entry_floats(c, 0), d.entry_floats(c, 1) };
		GAS_HIP(c, gas_launch_zero_entries(c->stream, dev.pool, floats, reinterpret_cast<const uint32_t *>(p.d_upload + zoff), z));
	}
	GAS_HIP(c, hipStreamSynchronize(c->stream)); // the pinned staging buffer is reused by the next flush
	return GAS_OK;
}

// GAS_FLAG_BATCHED_LAUNCH: has the "basic" family settings waiting that recorded callbacks have not seen?  params_mu held.
bool fx_basic_dirty(const gas_ctx *c) {
	return !c->fx[FX_BASIC].dirty_list.empty();
}

} // namespace gas_priv

extern "C" {

int gas_fx_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_settings *settings, uint32_t n) {
	return fx_publish(c, FX_BASIC, slots, settings, n);
}

int gas_fx_dyn_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_dyn_settings *settings, uint32_t n) {
	return fx_publish(c, FX_DYN, slots, settings, n);
}

int gas_fx_line_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_line_settings *settings, uint32_t n) {
	return fx_publish(c, FX_LINES, slots, settings, n);
}

int gas_fx_eq_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_eq_settings *settings, uint32_t n) {
	return fx_publish(c, FX_EQ, slots, settings, n);
}

int gas_fx_mod_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_mod_settings *settings, uint32_t n) {
	return fx_publish(c, FX_MOD, slots, settings, n);
}

int gas_fx_stereo_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_stereo_settings *settings, uint32_t n) {
	return fx_publish(c, FX_STEREO, slots, settings, n);
}

int gas_fx_filter_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_filter_settings *settings, uint32_t n) {
	return fx_publish(c, FX_FILTER, slots, settings, n);
}

int gas_ctx_reserve_fx_lines(gas_ctx *c, uint32_t delay_lines, uint32_t reverb_lines) {
	return fx_reserve(c, FX_LINES, delay_lines, reverb_lines);
}

int gas_ctx_reserve_fx_eq(gas_ctx *c, uint32_t eq_banks) {
	return fx_reserve(c, FX_EQ, eq_banks, 0);
}

int gas_ctx_reserve_fx_mod(gas_ctx *c, uint32_t chorus_lines, uint32_t phaser_banks) {
	return fx_reserve(c, FX_MOD, chorus_lines, phaser_banks);
}

int gas_ctx_reserve_fx_stereo(gas_ctx *c, uint32_t enhance_rings) {
	return fx_reserve(c, FX_STEREO, enhance_rings, 0);
}

int gas_ctx_reserve_fx_filter(gas_ctx *c, uint32_t banks) {
	return fx_reserve(c, FX_FILTER, banks, 0);
}

} // extern "C"
