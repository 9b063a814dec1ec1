// gas_ctx.hip -- the C ABI of include/gas_amd.h: context, device-resident playback-data slots,
// parameter publication, and the per-callback launch sequence that stands in for
// AudioSpatializerInstance::_mix_from_playback_list (audio_spatializer.cpp:326-471).
// Entries off the callback path live in their own units behind gas_ctx_priv.h: gas_ctx_conv.hip (bus convolvers),
// gas_ctx_streams.hip (stream control, fed rows), gas_ctx_calc.hip (parameter generators), gas_ctx_hrtf_profile.hip.
//
// There is NO CPU fallback: every entry needs a HIP device and fails with GAS_ERR_NO_DEVICE /
// GAS_ERR_DEVICE otherwise.
#include "gas_ctx_priv.h"

namespace {

// The effect families (k_fx_families, below): which one carries an effect kind's settings (-1: none), and the stage of
// a staged chain that runs the kind.
int family_of(int kind);
hipError_t fx_launch(const gas_ctx *c, int kind, const gas_group_args &in, uint32_t chain_pos, gas_audio_frame *rows_out);

int group_of(int kind, const int32_t *fx, uint32_t n_fx) {
	if (kind == GAS_KIND_3D_MIX) {
		return n_fx == 0 ? G_3D_MIX : -1;
	}
	if (kind == GAS_KIND_3D_PROCESS) {
		return n_fx == 0 ? G_3D_PROCESS : -1;
	}
	if (kind != GAS_KIND_EFFECT) {
		return -1;
	}
	if (n_fx == 0) {
		return G_FX_COPY;
	}
	if (n_fx == 1 && fx[0] == GAS_FX_HIGHSHELF) {
		return G_FX_SHELF;
	}
	if (n_fx == 1 && fx[0] == GAS_FX_HRTF) {
		return G_FX_HRTF;
	}
	if (n_fx == 1 && fx[0] == GAS_FX_EARLY_REFLECTIONS) {
		return G_FX_ER;
	}
	if (n_fx == 2 && fx[0] == GAS_FX_EARLY_REFLECTIONS && fx[1] == GAS_FX_HRTF) {
		return G_FX_ER_HRTF;
	}
	// any other order / combination of the implemented effects runs staged; the per-slot state allows one early-
	// reflection ring and one HRTF history per playback
	int n_er = 0, n_hrtf = 0;
	for (uint32_t j = 0; j < n_fx; j++) {
		if (fx[j] != GAS_FX_HIGHSHELF && fx[j] != GAS_FX_EARLY_REFLECTIONS && fx[j] != GAS_FX_HRTF && family_of(fx[j]) < 0) {
			return -1;
		}
		n_er += fx[j] == GAS_FX_EARLY_REFLECTIONS;
		n_hrtf += fx[j] == GAS_FX_HRTF;
	}
	if (n_er > 1 || n_hrtf > 1) {
		return -2;
	}
	return G_FX_GENERIC;
}

// The plain [HRTF] chain runs in k_hrtf_uni (one uniform launch, exact peaks per source on request) unless a mode
// only k_hrtf_ols implements is on.
inline bool uni_ok(const gas_ctx *c) {
	return (c->cfg.flags & (GAS_FLAG_HRTF_CROSSFADE | GAS_FLAG_DIRECTION_RUNS | GAS_FLAG_DIRECTION_ORDER | GAS_FLAG_HRTF_INTERPOLATE)) == 0;
}

inline bool blend_on(const gas_ctx *c) {
	return (c->cfg.flags & GAS_FLAG_HRTF_INTERPOLATE) != 0;
}

inline bool fade_on(const gas_ctx *c) {
	return (c->cfg.flags & GAS_FLAG_HRTF_BLEND_FADE) != 0;
}

inline bool er_fade_on(const gas_ctx *c) {
	return (c->cfg.flags & GAS_FLAG_ER_TAP_FADE) != 0;
}

inline bool wants_peak(const gas_ctx *c, const SlotInfo &si) {
	return si.draining || !(c->cfg.flags & GAS_FLAG_PEAKS_DRAINING_ONLY);
}

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

// Effect kinds by chain position, 8 bits each, first effect in the low byte.  The digits keep their order, so sorting by
// signature orders chains of the kinds below 16 exactly as the earlier 4-bit digits did.
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

uint32_t chain_signature(const int32_t *fx, uint32_t n_fx) {
	uint32_t sig = 0;
	for (uint32_t j = 0; j < n_fx; j++) {
		sig |= (uint32_t)(fx[j] & 0xff) << (8 * j);
	}
	return sig;
}

bool chain_has(uint32_t sig, int kind) {
	for (int j = 0; j < 4; j++) {
		if (((sig >> (8 * j)) & 0xff) == kind) {
			return true;
		}
	}
	return false;
}

// A staged chain whose last effect is the HRTF (and that has a stage in front of it) hands that last stage to
// k_hrtf_uni over the previous stage's rows -- frequency-domain accumulation, one inverse pair per workgroup, exact
// peaks -- instead of k_hrtf_rows + k_rows_accumulate (per-source inverse pairs written out as rows and read back):
// [HIGHSHELF, HRTF], the reference example's shelf in front of the new effect, 62 -> 37 us at 8192 sources.
inline bool range_ends_in_uni(const ChainRange &r, bool staged_uni) {
	int last = 0, n_fx = 0;
	for (int j = 0; j < 4; j++) {
		const int kind = (r.sig >> (8 * j)) & 0xff;
		if (kind) {
			last = kind;
			n_fx++;
		}
	}
	return staged_uni && n_fx >= 2 && last == GAS_FX_HRTF;
}

inline uint32_t range_partials(const ChainRange &r, bool staged_uni) {
	return range_ends_in_uni(r, staged_uni) ? gas_hrtf_uni_partials(r.count) : gas_hrtf_partials(r.count);
}

// Partial mixes each launch group writes (must mirror the launchers' grids).
void plan_partials(const Group *groups, const std::vector<ChainRange> &ranges, uint32_t *pcount, bool uni_hrtf, bool staged_uni, bool uni_er) {
	for (int gt = 0; gt < G_COUNT; gt++) {
		pcount[gt] = 0;
	}
	for (int gt = G_3D_MIX; gt <= G_FX_SHELF; gt++) {
		pcount[gt] = groups[gt].count ? gas_biquad_partials(groups[gt].count) : 0;
	}
	pcount[G_FX_ER] = groups[G_FX_ER].count ? gas_hrtf_partials(groups[G_FX_ER].count) : 0;
	for (int gt : { (int)G_FX_HRTF, (int)G_FX_ER_HRTF }) {
		gas_hrtf_launch_plan p;
		gas_hrtf_plan(groups[gt].count, groups[gt + 1].count, &p);
		pcount[gt] = p.wgs_fd;
		pcount[gt + 1] = p.wgs_pk;
	}
	if (uni_hrtf && groups[G_FX_HRTF].count && !groups[G_FX_HRTF_PK].count) {
		pcount[G_FX_HRTF] = gas_hrtf_uni_partials(groups[G_FX_HRTF].count); // k_hrtf_uni's own grid
	}
	if (uni_er && groups[G_FX_ER_HRTF].count + groups[G_FX_ER_HRTF_PK].count) { // [ER, HRTF] in k_hrtf_uni<ER>: both groups in one list
		const int lead = groups[G_FX_ER_HRTF].count ? G_FX_ER_HRTF : G_FX_ER_HRTF_PK;
		pcount[G_FX_ER_HRTF] = pcount[G_FX_ER_HRTF_PK] = 0;
		pcount[lead] = gas_hrtf_uni_partials(groups[G_FX_ER_HRTF].count + groups[G_FX_ER_HRTF_PK].count);
	}
	if (groups[G_FX_GENERIC].count) {
		for (const ChainRange &r : ranges) {
			pcount[G_FX_GENERIC] += range_partials(r, staged_uni);
		}
	}
}

// B = N*F*8 + N*S + N*H + B_tab + C*F*8 (compulsory bytes of one launch group).
uint64_t group_bytes(const gas_ctx *c, int gt, uint32_t n) {
	const uint64_t F = c->cfg.frames;
	uint64_t C = 1, S = 0, H = 0, tab = 0;
	switch (gt) {
		case G_3D_MIX:
			C = c->cfg.channel_count;
			S = C * 144 + 32 + 8; // 2 ears x (9 f32 r + 9 f32 w) per pair + params + peak
			break;
		case G_3D_PROCESS:
		case G_FX_SHELF:
			S = 144 + 32 + 8;
			break;
		case G_FX_COPY:
			S = 8;
			break;
		case G_FX_HRTF:
		case G_FX_HRTF_PK:
			S = 24 + (blend_on(c) ? sizeof(gas_hrtf_blend) : 0) + (fade_on(c) ? 2 * sizeof(gas_hrtf_blend) : 0); // gain + dir, previous gain r/w, peak; the blend row; the previous effective row r/w
			H = 2ull * c->hist_len * 4; // history read + write
			tab = (uint64_t)c->tab.dirs * 2 * GAS_HRTF_TAPS * 4;
			break;
		case G_FX_ER:
			S = 8 + 64 + 8 + (er_fade_on(c) ? 2 * 64 : 0); // position r/w, taps, peak; GAS_FLAG_ER_TAP_FADE: the old tap row r/w
			H = (uint64_t)GAS_ER_TAPS * F * 8 + F * 8; // tap gathers + ring write (a fading source's second set of gathers re-reads the same ring: not compulsory bytes)
			break;
		case G_FX_ER_HRTF:
		case G_FX_ER_HRTF_PK:
			S = 24 + 64 + 8 + (blend_on(c) ? sizeof(gas_hrtf_blend) : 0) + (fade_on(c) ? 2 * sizeof(gas_hrtf_blend) : 0);
			H = (uint64_t)GAS_ER_TAPS * F * 8 + F * 8 + 2ull * c->hist_len * 4;
			tab = (uint64_t)c->tab.dirs * 2 * GAS_HRTF_TAPS * 4;
			break;
	}
	return (uint64_t)n * (F * 8 + S + H) + tab + C * F * 8;
}

int ensure_partials(gas_ctx *c, uint32_t rows) {
	if (rows <= c->partial_rows) {
		return GAS_OK;
	}
	if (c->d_partials) {
		GAS_HIP(c, hipStreamSynchronize(c->stream));
	}
	// two generations when the reduce is pipelined: callback t+1 fills one while callback t's is being summed; with
	// batched launches one per block being filled and one per block being summed
	c->partial_planes = c->pipelined_mix ? ((c->cfg.flags & GAS_FLAG_BATCHED_LAUNCH) != 0 ? 2u * GAS_HRTF_MULTI_MAX_BLOCKS : 2u) : 1u;
	GAS_HIP(c, c->mem.grow(c->d_partials, c->partial_rows, rows, (size_t)c->partial_planes * c->cfg.channel_count * c->cfg.frames * 2));
	return GAS_OK;
}

// The pending sums (GAS_FLAG_PIPELINED_MIX), c->pending: where one's partial mixes lie, what a launch that carries it
// is handed, and what the carrying adds to that launch's bytes.
inline float *partials_plane(const gas_ctx *c, int parity) {
	return c->d_partials + (size_t)parity * c->partial_rows * c->cfg.channel_count * c->cfg.frames * 2;
}

gas_deferred_reduce carried_job(const gas_ctx *c, const gas_ctx::PendingMix &pm) {
	gas_deferred_reduce job;
	job.partials = partials_plane(c, pm.parity);
	job.p_count = pm.p_total;
	job.elems = c->cfg.frames * 2;
	job.out = reinterpret_cast<float *>(pm.out);
	return job;
}

inline uint64_t carried_bytes(const gas_deferred_reduce &job) {
	return job.partials ? ((uint64_t)job.p_count + 1) * job.elems * sizeof(float) : 0;
}

// Launches the pending callback's k_mix_reduce on the context's stream.
int reduce_now(gas_ctx *c, const gas_ctx::PendingMix &pm) {
	GAS_HIP(c, gas_launch_mix_reduce(c->stream, partials_plane(c, pm.parity), pm.p_total, c->partial_rows, 1, c->cfg.frames, pm.out));
	return GAS_OK;
}

} // namespace
namespace gas_priv __attribute__((visibility("hidden"))) {
int join_outputs(gas_ctx *c) {
	const std::vector<gas_ctx::PendingMix> all = std::move(c->pending);
	c->pending.clear();
	if (all.size() == 1) {
		return reduce_now(c, all[0]);
	}
	// the sums a batched launch left: one launch for all of them (eight k_mix_reduce launches cost 38 us)
	for (size_t i = 0; i < all.size(); i += GAS_HRTF_MULTI_MAX_BLOCKS) {
		gas_reduce_jobs jobs;
		for (size_t j = i; j < all.size() && j < i + GAS_HRTF_MULTI_MAX_BLOCKS; j++) {
			jobs.partials[jobs.count] = partials_plane(c, all[j].parity);
			jobs.p_count[jobs.count] = all[j].p_total;
			jobs.out[jobs.count] = reinterpret_cast<float *>(all[j].out);
			jobs.count++;
		}
		GAS_HIP(c, gas_launch_mix_reduce_jobs(c->stream, jobs, c->cfg.frames));
	}
	return GAS_OK;
}
} // namespace gas_priv
namespace {

// A plane of d_partials that no pending sum still reads and that is not in `taken`.
int free_plane(const gas_ctx *c, const std::vector<int> &taken) {
	for (int p = 0; p < (int)c->partial_planes; p++) {
		bool busy = false;
		for (const gas_ctx::PendingMix &pm : c->pending) {
			busy = busy || pm.parity == p;
		}
		for (int t : taken) {
			busy = busy || t == p;
		}
		if (!busy) {
			return p;
		}
	}
	return -1;
}

// Where a callback's rows come from: float rows, or "fused" -- none, the HRTF launch samples the bound streams itself.
struct RowSource {
	const gas_audio_frame *rows = nullptr; // [n][F]
	gas_cursor *cursors = nullptr; // non-null: fused, the slot-indexed cursor array
	const uint8_t *feed = nullptr; // fused only: the feed table when an entry of the list is fed (gas_source_feed_rows)
	bool fused() const {
		return cursors != nullptr;
	}
};

// One callback over already-grouped entries: everything run_groups is told.
struct RunArgs {
	RowSource src;
	const uint32_t *slots = nullptr; // [n_total] sorted by launch group
	const uint32_t *rows = nullptr; // [n_total] row of src (and of peaks) per entry, or nullptr (= identity)
	const Group *groups = nullptr; // [G_COUNT]
	const std::vector<ChainRange> *ranges = nullptr; // sub-runs of groups[G_FX_GENERIC]
	uint32_t n_total = 0;
	gas_audio_frame *out = nullptr;
	float *peaks = nullptr; // [n_total][2]
	uint32_t channel_begin = 0, channel_count = 1;
	int force_mode = -1; // >= 0: the 3D groups run this gas_biquad_mode
	bool use_order = false; // the context's cached processing orders (d_order) apply
	bool pipelined = false; // the sum may be left to the next callback (GAS_FLAG_PIPELINED_MIX)
	const gas_bus_args *buses = nullptr; // gas_process_block_buses over effect kinds: the staged chains' rows are mixed per bus
	const gas_params *fresh = nullptr; // device-published parameter rows in row order, not yet in the table: the HRTF launches read them and write them through
};

// A callback over the context's own cached list.
RunArgs own_list(const gas_ctx *c, const RowSource &src, uint32_t n, gas_audio_frame *out, float *peaks) {
	RunArgs a;
	a.src = src;
	a.slots = c->d_slots;
	a.rows = c->cached_identity_rows ? nullptr : c->d_rows;
	a.groups = c->groups;
	a.ranges = &c->chain_ranges;
	a.n_total = n;
	a.out = out;
	a.peaks = peaks;
	return a;
}

// The plain-[HRTF] group of the context's own list, for a launch that covers exactly it.
gas_group_args own_hrtf_group(const gas_ctx *c, const gas_audio_frame *src, uint32_t n, float *peaks) {
	const Group &gr = c->groups[G_FX_HRTF];
	gas_group_args ga;
	ga.src = src;
	ga.rows = c->cached_identity_rows ? nullptr : c->d_rows + gr.offset;
	ga.slots = gr.contiguous ? nullptr : c->d_slots + gr.offset; // a contiguous slot range needs no list on the device
	ga.slot_base = gr.contiguous ? gr.slot_base : 0;
	ga.n = n;
	ga.peaks = peaks;
	return ga;
}

// The fields every HRTF launch of this context shares.
gas_hrtf_launch_common hrtf_common(const gas_ctx *c) {
	gas_hrtf_launch_common k;
	k.stream = c->stream;
	k.st = &c->st;
	k.tab = &c->tab;
	k.twiddles = c->d_tw;
	k.frames = c->cfg.frames;
	k.hist_len = c->hist_len;
	k.fade_env = c->d_fade_env;
	return k;
}

// A biquad launch (gas_launch_biquad_mix: k_biquad_mix, or the form its launcher picks) over `g`, with the fields every
// such launch of this context shares: one channel pair from channel 0, partial rows in the context's stride.
gas_biquad_launch biquad_launch(const gas_ctx *c, int mode, const gas_group_args &g, float *partials, uint32_t p_offset) {
	gas_biquad_launch lb;
	lb.stream = c->stream;
	lb.mode = mode;
	lb.g = g;
	lb.st = &c->st;
	lb.frames = c->cfg.frames;
	lb.mix_rate = c->cfg.mix_rate;
	lb.partials = partials;
	lb.p_offset = p_offset;
	lb.p_stride = c->partial_rows;
	lb.scan_ok = c->sw.shelf_scan;
	lb.pipe_ok = c->sw.biquad_pipe;
	return lb;
}

// Which entries of the plain-[HRTF] group of the context's own list report their exact peak (build_groups): the bit
// list, unless all of them or none do.
inline const uint32_t *plain_peak_bits(const gas_ctx *c) {
	return c->uni_peak_any && !c->uni_peak_all ? c->d_peak_bits : nullptr;
}

// k_hrtf_uni over the plain-[HRTF] group `g` of the context's own list.
gas_hrtf_uni_launch plain_uni_launch(const gas_ctx *c, const gas_group_args &g, const RowSource &src, float *partials, uint32_t p_offset) {
	gas_hrtf_uni_launch lu{ hrtf_common(c) };
	lu.g = g;
	lu.peak_bits = plain_peak_bits(c);
	lu.peak_all = c->uni_peak_all;
	lu.partials = partials;
	lu.p_offset = p_offset;
	lu.cursors = src.cursors;
	lu.feed = src.feed;
	return lu;
}

// What run_groups' loop over the groups shares with the launch families below.
struct GroupRun {
	float *parts = nullptr; // this callback's plane of d_partials
	uint32_t p_off = 0; // its rows taken by the groups in front of the current one
	uint32_t p_total = 0; // ... and by all groups
	bool uni_hrtf = false, staged_uni = false, uni_er = false; // the launch forms plan_partials counted the rows of
	gas_deferred_reduce job; // the previous callback's sum (GAS_FLAG_PIPELINED_MIX), until a launch takes it along
	int carrier_gt = -1; // the frequency-domain group whose launch does
	// The job if fd_gt's launch is the carrier (`bytes`: what summing it adds to the launch's traffic), else none.
	gas_deferred_reduce take(int fd_gt, uint64_t &bytes) {
		if (fd_gt != carrier_gt) {
			return gas_deferred_reduce();
		}
		const gas_deferred_reduce taken = job;
		job = gas_deferred_reduce();
		bytes = carried_bytes(taken);
		return taken;
	}
};

// G_FX_HRTF / G_FX_ER_HRTF and the exact-peak group behind each: one launch covers both (`ga`: group gt's entries, the
// exact-peak group's when the frequency-domain one is empty).  k_hrtf_uni where it applies, else k_hrtf_ols.
int launch_hrtf_groups(gas_ctx *c, const RunArgs &a, int gt, const gas_group_args &ga, GroupRun &run, uint64_t &carried) {
	const Group *const groups = a.groups;
	const uint32_t *const d_slots = a.slots, *const d_rows = a.rows;
	const bool is_pk = gt == G_FX_HRTF_PK || gt == G_FX_ER_HRTF_PK;
	const int fd_gt = is_pk ? gt - 1 : gt;
	const Group &gr = groups[gt], &gp = groups[fd_gt + 1];
	gas_group_args g_fd = ga, g_pk = ga;
	if (is_pk) {
		g_fd.n = 0;
	} else {
		g_pk.rows = d_rows ? d_rows + gp.offset : nullptr;
		g_pk.slots = d_slots + gp.offset;
		g_pk.n = gp.count;
	}
	// contiguous slot ranges need no slot list on the device (one dependent load less in the prologue)
	if (g_fd.n && groups[fd_gt].contiguous) {
		g_fd.slots = nullptr;
		g_fd.slot_base = groups[fd_gt].slot_base;
	}
	if (g_pk.n && groups[fd_gt + 1].contiguous) {
		g_pk.slots = nullptr;
		g_pk.slot_base = groups[fd_gt + 1].slot_base;
	}
	const gas_params *fresh = a.fresh; // both HRTF forms read device-published rows themselves and write them through
	if (gt == G_FX_HRTF && gp.count == 0 && run.uni_hrtf) {
		// the whole plain-[HRTF] group in one uniform launch (k_hrtf_uni.hip)
		// XCD-affine processing order (k_xcd_order): rebuilt when the list or any parameter changed, else reused
		const uint32_t uni_wgs = gas_hrtf_uni_partials(g_fd.n);
		c->last_uni_ordered = false;
		if (a.use_order && ((c->cfg.flags & GAS_FLAG_XCD_ORDER) != 0 || g_fd.n >= c->sw.xcd_order_auto_min) && uni_wgs % 8 == 0 && c->tab.dirs >= 8) {
			GAS_HIP(c, alloc_once(c, c->d_order, c->cfg.max_sources));
			uint32_t *ord = c->d_order + groups[fd_gt].offset;
			if (!c->order_ok[fd_gt]) {
				GAS_HIP(c, gas_launch_xcd_order(c->stream, g_fd, c->st.params, fresh, c->tab.dirs, uni_wgs, gas_hrtf_uni_waves(), ord));
				c->order_ok[fd_gt] = true;
			}
			g_fd.order = ord;
			c->last_uni_ordered = true;
		}
		gas_hrtf_uni_launch lu = plain_uni_launch(c, g_fd, a.src, run.parts, run.p_off);
		lu.fresh = fresh;
		lu.job = run.take(fd_gt, carried); // (a pending sum makes this group the carrier: it is the first of the two)
		GAS_HIP(c, gas_launch_hrtf_uni(lu));
		return GAS_OK;
	}
	if (fd_gt == G_FX_ER_HRTF && run.uni_er) {
		gas_group_args gu = ga; // this group's entries, then (frequency-domain group first) the exact-peak group's
		gu.n = is_pk ? gr.count : gr.count + gp.count;
		const bool whole = gr.contiguous && (is_pk || gp.count == 0 || (gp.contiguous && gp.slot_base == gr.slot_base + gr.count));
		if (whole) {
			gu.slots = nullptr;
			gu.slot_base = gr.slot_base;
		}
		gas_hrtf_uni_launch lu{ hrtf_common(c) };
		lu.g = gu;
		lu.peak_all = is_pk;
		lu.partials = run.parts;
		lu.p_offset = run.p_off;
		lu.fresh = fresh;
		lu.job = run.take(fd_gt, carried);
		lu.er_ring_frames = c->cfg.er_ring_frames;
		lu.peak_from = is_pk ? 0u : gr.count;
		GAS_HIP(c, gas_launch_hrtf_uni(lu));
		return GAS_OK;
	}
	// GAS_FLAG_DIRECTION_ORDER: direction order of the frequency-domain group, rebuilt when the
	// callback's list or any parameter changed, else reused.  Only when directions repeat within a segment.
	if (a.use_order && (c->cfg.flags & GAS_FLAG_DIRECTION_ORDER) != 0 && g_fd.n >= GAS_DIR_ORDER_MIN_SOURCES && (c->cfg.flags & GAS_FLAG_HRTF_CROSSFADE) == 0 && gas_dir_order_supported(c->tab.dirs)) {
		const uint32_t seg = g_fd.n < GAS_DIR_ORDER_SEGMENT ? g_fd.n : GAS_DIR_ORDER_SEGMENT;
		if (seg >= 2 * c->tab.dirs) {
			GAS_HIP(c, alloc_once(c, c->d_order, c->cfg.max_sources));
			uint32_t *ord = c->d_order + groups[fd_gt].offset;
			if (!c->order_ok[fd_gt]) {
				GAS_HIP(c, gas_launch_dir_order(c->stream, g_fd, c->st.params, fresh, c->tab.dirs, ord));
				c->order_ok[fd_gt] = true;
			}
			g_fd.order = ord;
		}
	}
	gas_hrtf_ols_launch lo{ hrtf_common(c) };
	lo.with_er = fd_gt == G_FX_ER_HRTF;
	lo.crossfade = (c->cfg.flags & GAS_FLAG_HRTF_CROSSFADE) != 0;
	lo.runs = (c->cfg.flags & (GAS_FLAG_DIRECTION_RUNS | GAS_FLAG_DIRECTION_ORDER)) != 0;
	lo.g_fd = g_fd;
	lo.g_pk = g_pk;
	lo.er_ring_frames = c->cfg.er_ring_frames;
	lo.partials = run.parts;
	lo.p_offset = run.p_off;
	lo.cursors = fd_gt == G_FX_HRTF ? a.src.cursors : nullptr;
	lo.fresh = fresh;
	lo.job = run.take(fd_gt, carried);
	lo.blend = blend_on(c);
	lo.fade = fade_on(c);
	GAS_HIP(c, gas_launch_hrtf_ols(lo));
	return GAS_OK;
}

// G_FX_GENERIC: audio_spatializer_effect.cpp:52-76 on the device, chain by chain (`ga`: the group's entries).  Effect j
// reads the previous stage's rows and writes the other ping-pong buffer; the last stage's rows are mixed by
// k_rows_accumulate, unless the chain ends in a k_hrtf_uni launch, which mixes by itself.
int launch_staged_chains(gas_ctx *c, const RunArgs &a, const gas_group_args &ga, const GroupRun &run) {
	const uint32_t F = c->cfg.frames;
	const Group &gr = a.groups[G_FX_GENERIC];
	const uint32_t *const d_slots = a.slots, *const d_rows = a.rows;
	const gas_audio_frame *const d_src = a.src.rows;
	size_t need = 0;
	for (const ChainRange &r : *a.ranges) {
		need = need > (size_t)r.count * F ? need : (size_t)r.count * F;
	}
	if (need > c->d_chain_frames) {
		GAS_HIP(c, hipStreamSynchronize(c->stream));
		size_t cap[2] = { c->d_chain_frames, c->d_chain_frames };
		c->d_chain_frames = 0; // both rows or neither
		GAS_HIP(c, c->mem.grow(c->d_chain[0], cap[0], need));
		GAS_HIP(c, c->mem.grow(c->d_chain[1], cap[1], need));
		c->d_chain_frames = need;
	}
	uint32_t pp = run.p_off;
	for (const ChainRange &r : *a.ranges) {
		const uint32_t off = gr.offset + r.offset, pp_r = pp;
		pp += range_partials(r, run.staged_uni);
		gas_group_args in = ga;
		in.n = r.count;
		in.slots = d_slots + off;
		in.rows = d_rows ? d_rows + off : nullptr;
		in.src = d_rows ? d_src : d_src + (size_t)off * F; // identity rows: the run's first row is entry `off`
		in.peaks = d_rows ? a.peaks : a.peaks + (size_t)off * 2;
		const uint32_t *peak_rows = in.rows;
		const bool last_is_uni = range_ends_in_uni(r, run.staged_uni);
		const bool own = a.groups == c->groups; // the context's own list: GAS_FLAG_PEAKS_DRAINING_ONLY's bits exist
		const int k0 = r.sig & 0xff;
		// a last stage that is k_hrtf_uni: exact peaks for every source of the chain, or (GAS_FLAG_PEAKS_DRAINING_ONLY,
		// the context's own list) for the draining ones
		gas_hrtf_uni_launch lu{ hrtf_common(c) };
		lu.peak_bits = own && r.peak_any && !r.peak_all ? c->d_peak_bits + (c->cfg.max_sources + 31) / 32 : nullptr;
		lu.peak_all = !own || r.peak_all;
		lu.partials = run.parts;
		lu.p_offset = pp_r;
		lu.peak_bit_base = r.offset;
		if (last_is_uni && c->sw.uni_flt && (r.sig >> 8) == GAS_FX_HRTF && (k0 == GAS_FX_HIGHSHELF || (k0 >= GAS_FX_LOWPASS && k0 <= GAS_FX_LOWSHELF)) && gas_shelf_scan_applies(c->sw.shelf_scan, k0 == GAS_FX_HIGHSHELF ? GAS_MODE_FX_HIGHSHELF : GAS_MODE_FX_FILTER, r.count, F)) {
			// [one-biquad filter, HRTF]: one launch (k_hrtf_uni<FLT>), no rows in between.  The filter there is the
			// scan form, so it is taken exactly where the two-launch road would take k_shelf_scan (same bits either
			// way; small callbacks and GAS_SHELF_SCAN=0 keep the engine's serial order)
			lu.g = in;
			lu.flt_kind = (uint32_t)k0;
			lu.mix_rate = c->cfg.mix_rate;
			GAS_HIP(c, gas_launch_hrtf_uni(lu));
			continue;
		}
		for (int j = 0; j < 4; j++) {
			const int kind = (r.sig >> (8 * j)) & 0xff;
			if (!kind) {
				break;
			}
			if (last_is_uni && c->uni_er_enabled && kind == GAS_FX_EARLY_REFLECTIONS && j < 3 && ((r.sig >> (8 * (j + 1))) & 0xff) == GAS_FX_HRTF) {
				// ... [ER, HRTF] at the end of a longer chain: both in the last launch (k_hrtf_uni<ER>), no rows in between
				lu.g = in;
				lu.g.peak_rows = peak_rows;
				lu.er_ring_frames = c->cfg.er_ring_frames;
				GAS_HIP(c, gas_launch_hrtf_uni(lu));
				break;
			}
			if (last_is_uni && kind == GAS_FX_HRTF) { // (the last effect: one HRTF per chain)
				lu.g = in; // dense rows of the previous stage, peaks into the callback's rows
				lu.g.peak_rows = peak_rows;
				GAS_HIP(c, gas_launch_hrtf_uni(lu));
				break;
			}
			gas_audio_frame *outb = c->d_chain[j & 1];
			if (kind == GAS_FX_HIGHSHELF) {
				gas_biquad_launch lb = biquad_launch(c, GAS_MODE_FX_HIGHSHELF, in, run.parts, 0);
				lb.channel_begin = (uint32_t)j;
				lb.rows_out = reinterpret_cast<float *>(outb);
				GAS_HIP(c, gas_launch_biquad_mix(lb));
			} else if (kind == GAS_FX_EARLY_REFLECTIONS) {
				GAS_HIP(c, gas_launch_er_only(c->stream, in, c->st, F, c->cfg.er_ring_frames, run.parts, 0, c->partial_rows, outb, er_fade_on(c)));
			} else if (kind == GAS_FX_HRTF) {
				GAS_HIP(c, gas_launch_hrtf_rows(c->stream, (c->cfg.flags & GAS_FLAG_HRTF_CROSSFADE) != 0, in, c->st, c->tab, c->d_tw, F, outb, blend_on(c), fade_on(c)));
			} else { // a family's kind: settings (and state, or the slot's pool entry) of chain position j
				GAS_HIP(c, fx_launch(c, kind, in, (uint32_t)j, outb));
			}
			in.src = outb; // dense rows from here on
			in.rows = nullptr;
		}
		if (last_is_uni) {
			continue;
		}
		gas_group_args fin = in;
		fin.rows = peak_rows; // peaks go to the callback's row of each source
		if (a.buses) {
			GAS_HIP(c, gas_launch_rows_accumulate_buses(c->stream, fin, F, a.buses->routes, a.buses->n_buses, run.p_total, run.parts, pp_r));
		} else {
			GAS_HIP(c, gas_launch_rows_accumulate(c->stream, fin, F, run.parts, pp_r));
		}
	}
	return GAS_OK;
}

// Device work of one callback over already-grouped entries.
int run_groups(gas_ctx *c, const RunArgs &a) {
	const uint32_t F = c->cfg.frames;
	const Group *const groups = a.groups;
	uint32_t pcount[G_COUNT];
	GroupRun run;
	run.uni_hrtf = groups == c->groups && uni_ok(c);
	run.staged_uni = uni_ok(c) && a.buses == nullptr && gas_hrtf_uni_waves() == 8; // staged chains ending in the HRTF: last stage = k_hrtf_uni
	// [ER, HRTF] through k_hrtf_uni<ER> (22.5 -> see profiles/r03_notes.md): the exact-peak group's entries follow the
	// frequency-domain group's in the callback's list, so one launch covers both
	const bool pipelined = a.pipelined && c->pipelined_mix && a.channel_count == 1 && c->cfg.channel_count == 1;
	const bool uni_er_pays = c->sw.uni_er_mode == 2 || groups[G_FX_ER_HRTF_PK].count * 4 <= groups[G_FX_ER_HRTF].count + groups[G_FX_ER_HRTF_PK].count;
	run.uni_er = uni_ok(c) && a.buses == nullptr && gas_hrtf_uni_waves() == 8 && c->uni_er_enabled && uni_er_pays && (groups[G_FX_ER_HRTF].count == 0 || groups[G_FX_ER_HRTF_PK].count == 0 || groups[G_FX_ER_HRTF].offset + groups[G_FX_ER_HRTF].count == groups[G_FX_ER_HRTF_PK].offset);
	plan_partials(groups, *a.ranges, pcount, run.uni_hrtf, run.staged_uni, run.uni_er);
	uint32_t p_total = 0, p_mix = 0;
	for (int gt = 0; gt < G_COUNT; gt++) {
		p_total += pcount[gt];
		if (gt == G_3D_MIX) {
			p_mix = p_total;
		}
	}
	run.p_total = p_total;
	// GAS_FLAG_PIPELINED_MIX: only callbacks that are one channel pair wide and carry an HRTF launch defer their sum
	// A launch can carry the pending sum when it is the plain [HRTF] kernel (register budget), covers every output
	// column with a workgroup and the pending callback left at most 256 partial rows (k_hrtf_ols: job_issue).
	// The plain [HRTF] launch takes it when there is one, else the [ER, HRTF] launch.
	bool carrier = false;
	if (!a.src.fused() && (c->cfg.flags & (GAS_FLAG_HRTF_CROSSFADE | GAS_FLAG_HRTF_INTERPOLATE)) == 0) {
		for (int gt : { (int)G_FX_HRTF, (int)G_FX_ER_HRTF }) {
			if (run.carrier_gt < 0 && groups[gt].count + groups[gt + 1].count > 0) {
				run.carrier_gt = gt;
			}
		}
	}
	if (run.carrier_gt >= 0) {
		// the oldest pending sum is the one a single launch carries; with none pending the launch counts as fitting (the
		// join below then has nothing to do either way)
		const bool fits = c->pending.empty() || c->pending.front().p_total <= 256;
		carrier = (pcount[run.carrier_gt] + pcount[run.carrier_gt + 1]) * GAS_HRTF_JOB_WAVES >= F * 2 / 4 && fits;
	}
	if (c->pending.size() > 1) { // left by a batched launch: a single launch carries one sum only, the oldest
		const std::vector<gas_ctx::PendingMix> more(c->pending.begin() + 1, c->pending.end());
		c->pending.resize(1);
		for (const gas_ctx::PendingMix &pm : more) {
			GAS_TRY(reduce_now(c, pm));
		}
	}
	if (!pipelined || !carrier || (p_total > 0 ? p_total : 1) > c->partial_rows) {
		GAS_TRY(join_outputs(c)); // nobody to carry the pending sum (or the partials are about to move): do it now
	}
	GAS_TRY(ensure_partials(c, (p_total > 0 ? p_total : 1) * (a.buses ? a.buses->n_buses : 1u))); // buses: p_total rows per bus, bus after bus
	const int parity = pipelined ? free_plane(c, {}) : 0;
	float *const parts = run.parts = partials_plane(c, parity);
	if (!c->pending.empty()) { // handed to the carrier's launch
		run.job = carried_job(c, c->pending.front());
		c->pending.clear();
	}
	// only the mix_channel launch over several channel pairs accumulates peaks (atomicMax over the pairs, from zero);
	// every other launch -- a single pair included -- stores them, so the zeroing pass (a 4 us dispatch) is skipped
	if (groups[G_3D_MIX].count + groups[G_3D_PROCESS].count > 0 && a.channel_count > 1 && a.force_mode != GAS_MODE_PROCESS_FRAMES) {
		GAS_HIP(c, hipMemsetAsync(a.peaks, 0, (size_t)a.n_total * 2 * sizeof(float), c->stream));
	}

	// the dominant launch of this callback is the one timed by the profiler
	int dom = -1;
	for (int gt = 0; gt < G_COUNT; gt++) {
		if (groups[gt].count > 0 && (dom < 0 || groups[gt].count > groups[dom].count)) {
			dom = gt;
		}
	}
	if ((dom == G_FX_HRTF_PK || dom == G_FX_ER_HRTF_PK) && groups[dom - 1].count > 0) {
		dom = dom - 1; // one launch covers both
	}

	for (int gt = 0; gt < G_COUNT; gt++) {
		const Group &gr = groups[gt];
		if (gr.count == 0) {
			continue;
		}
		gas_group_args ga;
		ga.src = a.src.rows; // nullptr when fused: only plain-[HRTF] launches run then, and they sample
		ga.rows = a.rows ? a.rows + gr.offset : nullptr;
		ga.slots = a.slots + gr.offset;
		ga.slot_base = 0;
		ga.n = gr.count;
		ga.peaks = a.peaks;
		const bool timed = gt == dom && c->prof.room() && c->prof.due();
		if (timed) {
			GAS_HIP(c, c->prof.begin(c->stream));
		}
		uint64_t carried = 0; // bytes of the previous callback's partial mixes summed inside this launch (GAS_FLAG_PIPELINED_MIX)
		switch (gt) {
			case G_3D_MIX:
			case G_3D_PROCESS: {
				int mode = gt == G_3D_MIX ? GAS_MODE_MIX_CHANNEL : GAS_MODE_PROCESS_FRAMES;
				if (a.force_mode >= 0) {
					mode = a.force_mode;
				}
				gas_biquad_launch lb = biquad_launch(c, mode, ga, parts, run.p_off);
				if (mode == GAS_MODE_MIX_CHANNEL) {
					lb.channel_begin = a.channel_begin;
					lb.channel_count = a.channel_count;
				}
				GAS_HIP(c, gas_launch_biquad_mix(lb));
			} break;
			case G_FX_COPY:
				GAS_HIP(c, gas_launch_biquad_mix(biquad_launch(c, GAS_MODE_COPY, ga, parts, run.p_off)));
				break;
			case G_FX_SHELF:
				GAS_HIP(c, gas_launch_biquad_mix(biquad_launch(c, GAS_MODE_FX_HIGHSHELF, ga, parts, run.p_off)));
				break;
			case G_FX_ER:
				GAS_HIP(c, gas_launch_er_only(c->stream, ga, c->st, F, c->cfg.er_ring_frames, parts, run.p_off, c->partial_rows, nullptr, er_fade_on(c)));
				break;
			case G_FX_HRTF_PK:
			case G_FX_ER_HRTF_PK:
				if (groups[gt - 1].count > 0) {
					break; // rode along with the frequency-domain group's launch
				}
				[[fallthrough]];
			case G_FX_HRTF:
			case G_FX_ER_HRTF:
				GAS_TRY(launch_hrtf_groups(c, a, gt, ga, run, carried));
				break;
			case G_FX_GENERIC:
				GAS_TRY(launch_staged_chains(c, a, ga, run));
				break;
		}
		if (timed) {
			GAS_HIP(c, c->prof.end(c->stream));
			c->prof.bytes = group_bytes(c, gt, gr.count) + carried;
			c->prof.k = 1;
			if ((gt == G_FX_HRTF || gt == G_FX_ER_HRTF) && groups[gt + 1].count > 0) {
				// the exact-peak sources ride in the same launch: add their per-source bytes (table/mix terms counted once)
				c->prof.bytes += group_bytes(c, gt + 1, groups[gt + 1].count) - group_bytes(c, gt + 1, 0);
			}
			c->prof.group = gt;
			c->prof.uni = (gt == G_FX_HRTF && run.uni_hrtf && groups[G_FX_HRTF_PK].count == 0) || ((gt == G_FX_ER_HRTF || gt == G_FX_ER_HRTF_PK) && run.uni_er);
			c->prof.multi = false;
			c->prof.pipe = (gt == G_3D_MIX || gt == G_3D_PROCESS || gt == G_FX_SHELF) && gas_biquad_uses_pipe(c->sw.biquad_pipe, gt == G_FX_SHELF ? GAS_MODE_FX_HIGHSHELF : (a.force_mode >= 0 ? a.force_mode : (gt == G_3D_MIX ? GAS_MODE_MIX_CHANNEL : GAS_MODE_PROCESS_FRAMES)), gr.count, gt == G_3D_MIX ? a.channel_count : 1, F, false);
		}
		run.p_off += pcount[gt];
	}

	// channel pair 0 sums every group's partials; pairs > 0 only the mix_channel group's (which come first)
	if (run.job.partials) { // no launch took the pending sum along (cannot happen with hrtf_launch set; kept for safety)
		GAS_HIP(c, gas_launch_mix_reduce(c->stream, run.job.partials, run.job.p_count, c->partial_rows, 1, F, reinterpret_cast<gas_audio_frame *>(run.job.out)));
	}
	if (pipelined) { // summed by the next callback's HRTF launch, gas_ctx_join_outputs or the next ordered call
		gas_ctx::PendingMix pm;
		pm.parity = parity;
		pm.p_total = p_total;
		pm.out = a.out;
		c->pending.push_back(pm);
		c->pipe_tick++;
		return GAS_OK;
	}
	if (a.buses) { // out[b][F]: bus b's rows are [b * p_total, (b + 1) * p_total)
		GAS_HIP(c, gas_launch_mix_reduce(c->stream, parts, p_total, p_total > 0 ? p_total : 1, a.buses->n_buses, F, a.out));
		return GAS_OK;
	}
	GAS_HIP(c, gas_launch_mix_reduce(c->stream, parts, p_total, c->partial_rows, 1, F, a.out));
	if (a.channel_count > 1) {
		GAS_HIP(c, gas_launch_mix_reduce(c->stream, parts + (size_t)c->partial_rows * F * 2, p_mix, c->partial_rows, a.channel_count - 1, F, a.out + F));
	}
	return GAS_OK;
}

int run_hrtf_batch(gas_ctx *c, const std::vector<gas_ctx::Deferred> &blocks, uint32_t n);

} // namespace
namespace gas_priv __attribute__((visibility("hidden"))) {
// GAS_FLAG_BATCHED_LAUNCH: the waiting callbacks run now -- something is about to change what they must see, or somebody
// wants their outputs.  The list, the groups and the parameter table are still the ones they were recorded with.
int flush_deferred(gas_ctx *c) {
	if (c->deferred.empty()) {
		return GAS_OK;
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device)); // callers flush before they do anything else, device selection included
	const std::vector<gas_ctx::Deferred> blocks = std::move(c->deferred);
	c->deferred.clear();
	if (blocks.size() > 1) {
		return run_hrtf_batch(c, blocks, c->deferred_n);
	}
	const gas_ctx::Deferred &d = blocks[0]; // a single one: k_hrtf_uni, exactly as the unbatched mode
	RowSource src;
	src.rows = d.src;
	RunArgs a = own_list(c, src, c->deferred_n, d.out, d.peaks);
	a.channel_count = c->cfg.channel_count;
	a.use_order = a.pipelined = true;
	a.fresh = d.fresh;
	return run_groups(c, a);
}
} // namespace gas_priv
namespace {

// Can this callback (already validated, groups built) wait for / run with its neighbours?
bool batchable(const gas_ctx *c, uint32_t n, bool fused) {
	if ((c->cfg.flags & GAS_FLAG_BATCHED_LAUNCH) == 0 || c->batch_depth < 2 || !c->pipelined_mix || c->cfg.channel_count != 1 || !uni_ok(c) || fused || (c->cfg.flags & GAS_FLAG_XCD_ORDER) != 0) {
		return false;
	}
	for (int gt = 0; gt < G_COUNT; gt++) {
		if (gt != G_FX_HRTF && c->groups[gt].count != 0) {
			return false;
		}
	}
	const uint32_t wgs = gas_hrtf_uni_partials(n);
	// every wave of the launch has a source; every output column of a carried sum finds a job wave
	return c->groups[G_FX_HRTF].count == n && n >= wgs * gas_hrtf_uni_waves() && wgs * GAS_HRTF_JOB_WAVES >= c->cfg.frames * 2 / 4 && wgs <= 256;
}

// 2 .. GAS_HRTF_MULTI_MAX_BLOCKS consecutive callbacks of the current list in ONE k_hrtf_multi launch.
int run_hrtf_batch(gas_ctx *c, const std::vector<gas_ctx::Deferred> &blocks, uint32_t n) {
	const uint32_t F = c->cfg.frames, K = (uint32_t)blocks.size();
	const uint32_t wgs = gas_hrtf_uni_partials(n);
	bool tall = false;
	for (const gas_ctx::PendingMix &pm : c->pending) {
		tall = tall || pm.p_total > 256;
	}
	if (wgs > c->partial_rows || c->partial_planes < 2 * GAS_HRTF_MULTI_MAX_BLOCKS || tall) {
		GAS_TRY(join_outputs(c)); // the partials are about to move, or a pending sum is too tall for a job wave
	}
	GAS_TRY(ensure_partials(c, wgs));
	const gas_group_args ga = own_hrtf_group(c, blocks[0].src, n, blocks[0].peaks);
	gas_hrtf_blocks mb;
	mb.k = K;
	for (uint32_t b = 0; b < K; b++) {
		mb.src[b] = blocks[b].src;
		mb.fresh[b] = blocks[b].fresh;
		mb.peaks[b] = blocks[b].peaks;
		if (blocks[b].fresh) {
			mb.last_fresh = blocks[b].fresh;
		}
	}
	// the pending sums ride with the first blocks of this launch, one each; any beyond that are summed right away
	uint64_t carried = 0;
	for (size_t j = 0; j < c->pending.size(); j++) {
		if (j < K) {
			mb.job[j] = carried_job(c, c->pending[j]);
			carried += carried_bytes(mb.job[j]);
		} else {
			GAS_TRY(reduce_now(c, c->pending[j]));
		}
	}
	// the planes this launch fills: none that a carried sum still reads (the pending records stay in place until the
	// planes are chosen)
	std::vector<int> planes;
	for (uint32_t b = 0; b < K; b++) {
		const int pl = free_plane(c, planes);
		if (pl < 0) {
			return GAS_ERR_DEVICE; // cannot happen: <= MAX carried + MAX filled of 2 MAX planes
		}
		planes.push_back(pl);
		mb.p_offset[b] = (uint32_t)pl * c->partial_rows * c->cfg.channel_count;
	}
	c->pending.clear();
	const bool timed = c->prof.room() && c->prof.due();
	if (timed) {
		GAS_HIP(c, c->prof.begin(c->stream));
	}
	GAS_HIP(c, gas_launch_hrtf_multi(c->stream, ga, mb, plain_peak_bits(c), c->uni_peak_all, c->st, c->tab, c->d_tw, F, c->hist_len, c->d_partials));
	if (timed) {
		GAS_HIP(c, c->prof.end(c->stream));
		// What this launch has to move (not K times the single-callback formula: k_hrtf_multi<., true> reads a history
		// row in its first block and writes it back in its last one, and meets the HRIR table once): per block the
		// frames, 8 B of peak per source, 8 B of (gain, direction) where the block has device-published rows, and the
		// workgroups' partial mix is not counted (round 2 did not either); once per launch the previous gain (r + w)
		// and the table; the history once in and once out, or per block when it cannot stay in LDS.
		{
			const uint64_t hist_rw = 2ull * c->hist_len * 4;
			const bool hist_lds = gas_hrtf_multi_hist_in_lds(n, F);
			uint64_t fresh_blocks = 0;
			for (uint32_t b = 0; b < K; b++) {
				fresh_blocks += blocks[b].fresh ? 1 : 0;
			}
			c->prof.bytes = (uint64_t)K * n * (F * 8 + 8) + fresh_blocks * n * 8 + (uint64_t)n * 8 + (hist_lds ? 1ull : (uint64_t)K) * n * hist_rw + (uint64_t)c->tab.dirs * 2 * GAS_HRTF_TAPS * 4 + (uint64_t)K * c->cfg.channel_count * F * 8 + carried;
		}
		c->prof.bytes_formula = (uint64_t)K * group_bytes(c, G_FX_HRTF, n) + carried;
		c->prof.k = K;
		c->prof.group = G_FX_HRTF;
		c->prof.uni = false;
		c->prof.pipe = false;
		c->prof.multi = true;
	}
	for (uint32_t b = 0; b < K; b++) {
		gas_ctx::PendingMix pm;
		pm.parity = planes[b];
		pm.p_total = wgs;
		pm.out = blocks[b].out;
		c->pending.push_back(pm);
	}
	c->pipe_tick += K;
	return GAS_OK;
}

// Marks row s of a slot-indexed host mirror for the next flush; params_mu held.
inline void mark_dirty(std::vector<uint8_t> &flag, std::vector<uint32_t> &list, uint32_t s) {
	if (!flag[s]) {
		flag[s] = 1;
		list.push_back(s);
	}
}

} // namespace
namespace gas_priv __attribute__((visibility("hidden"))) {
// Scatter a deferred device-side publish into the table (list unchanged since it was recorded).
int flush_pending_params(gas_ctx *c) {
	if (!c->pending_params) {
		return GAS_OK;
	}
	const gas_params *p = c->pending_params;
	c->pending_params = nullptr;
	GAS_HIP(c, gas_launch_scatter_params(c->stream, c->st.params, p, c->cached_identity_rows ? c->d_slots : c->d_slots_rows, c->pending_n));
	return GAS_OK;
}

// gas_hrtf_blend_publish's rows (and the all-zero rows of freed slots) -> the slot-indexed device table.  Control-rate
// data: one 32-byte copy per changed slot out of a pinned staging array, no kernel.
int flush_hrtf_blend(gas_ctx *c) {
	if (!blend_on(c)) {
		return GAS_OK;
	}
	uint32_t m = 0;
	{
		std::lock_guard<std::mutex> lk(c->params_mu);
		m = (uint32_t)c->blend_dirty_list.size();
		if (m == 0) {
			return GAS_OK;
		}
		if (alloc_once(c, c->h_blend_upload, c->cfg.max_sources, Mem::PINNED) != hipSuccess) {
			return GAS_ERR_OUT_OF_MEMORY;
		}
		for (uint32_t i = 0; i < m; i++) {
			const uint32_t s = c->blend_dirty_list[i];
			c->h_blend_upload[i] = c->h_blend[s];
			c->h_upload_slots[i] = s; // (the uploads above have been waited for)
			c->blend_dirty_flag[s] = 0;
		}
		c->blend_dirty_list.clear();
	}
	for (uint32_t i = 0; i < m; i++) {
		GAS_HIP(c, hipMemcpyAsync(c->st.hrtf_blend + c->h_upload_slots[i], c->h_blend_upload + i, sizeof(gas_hrtf_blend), hipMemcpyHostToDevice, c->stream));
	}
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	return GAS_OK;
}
} // namespace gas_priv
namespace {

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

int family_of(int kind) {
	return kind >= 0 && kind < 256 ? k_fx_kinds.family[kind] : -1;
}

hipError_t fx_launch(const gas_ctx *c, int kind, const gas_group_args &in, uint32_t chain_pos, gas_audio_frame *rows_out) {
	const int f = family_of(kind);
	return f < 0 ? hipErrorInvalidValue : k_fx_families[f].launch(c, kind, in, chain_pos, rows_out);
}

std::array<int32_t, GAS_MAX_EFFECTS> fx_no_entries() {
	std::array<int32_t, GAS_MAX_EFFECTS> none;
	none.fill(-1);
	return none;
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
		p.h_of.assign(c->cfg.max_sources, fx_no_entries());
		p.h_settings = std::move(defaults);
		p.dirty_flag.assign(c->cfg.max_sources, 0);
	}
	return GAS_OK;
}

} // namespace
namespace gas_priv __attribute__((visibility("hidden"))) {
// Host-published gas_params rows -> the slot-indexed device table.
int flush_param_rows(gas_ctx *c) {
	uint32_t m = 0;
	{
		std::lock_guard<std::mutex> lk(c->params_mu);
		m = (uint32_t)c->dirty_list.size();
		for (uint32_t i = 0; i < m; i++) {
			const uint32_t s = c->dirty_list[i];
			c->h_upload[i] = c->h_params[s];
			c->h_upload_slots[i] = s;
			c->dirty_flag[s] = 0;
		}
		c->dirty_list.clear();
	}
	if (m > 0) {
		// the pinned upload buffers are reused next callback: the copies must have left the host first
		GAS_HIP(c, hipMemcpyAsync(c->d_upload, c->h_upload, (size_t)m * sizeof(gas_params), hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, hipMemcpyAsync(c->d_upload_slots, c->h_upload_slots, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, gas_launch_scatter_params(c->stream, c->st.params, c->d_upload, c->d_upload_slots, m));
		GAS_HIP(c, hipStreamSynchronize(c->stream));
	}
	return GAS_OK;
}
} // namespace gas_priv
namespace {

int flush_params(gas_ctx *c) {
	int rc = flush_param_rows(c);
	rc = rc != GAS_OK ? rc : fx_flush(c, FX_BASIC); // (the blend rows keep their place between the first two families)
	rc = rc != GAS_OK ? rc : flush_hrtf_blend(c);
	for (int f = FX_BASIC + 1; f < FX_FAMILIES && rc == GAS_OK; f++) {
		rc = fx_flush(c, f);
	}
	return rc;
}

} // namespace
namespace gas_priv __attribute__((visibility("hidden"))) {
// gas_source_feed_rows: forget the slot's pending row.  Its bytes of the feed table stay taken until the next stream
// callback empties the table (or feed_place moves on to the table's other half).
void feed_drop(gas_ctx *c, uint32_t slot) {
	if (c->feed.word[slot] == GAS_FEED_NONE) {
		return;
	}
	c->feed.word[slot] = GAS_FEED_NONE;
	auto it = std::find(c->feed.slots.begin(), c->feed.slots.end(), slot);
	*it = c->feed.slots.back();
	c->feed.slots.pop_back();
}
} // namespace gas_priv
namespace {

// Frees requested on other threads become the audio thread's pending frees (deferred like audio_spatializer.cpp:538-547).
void adopt_frees(gas_ctx *c) {
	std::lock_guard<std::mutex> lk(c->alloc_mu);
	if (!c->free_inbox.empty()) {
		c->pending_free.insert(c->pending_free.end(), c->free_inbox.begin(), c->free_inbox.end());
		c->free_inbox.clear();
	}
}

int apply_pending_frees(gas_ctx *c) {
	adopt_frees(c);
	if (c->pending_free.empty()) {
		return GAS_OK;
	}
	bool had_stream = false;
	for (uint32_t s : c->pending_free) {
		had_stream = had_stream || c->streams.h_cursors[s].pcm != nullptr;
	}
	if (had_stream) {
		stream_rows_sync_back(c); // the compact mirror may still name these slots: fold it back before they are cleared
		c->streams.groups_gen = UINT64_MAX;
	}
	std::lock_guard<std::mutex> alloc_lk(c->alloc_mu);
	for (uint32_t s : c->pending_free) {
		SlotInfo &si = c->slots[s];
		for (int f = 0; f < FX_FAMILIES; f++) {
			fx_return_entries(c, f, s, si.chain_sig);
		}
		si = SlotInfo{};
		si.dirty_state = 1;
		if (blend_on(c)) { // the next playback in this slot starts without a blend: the all-zero row, uploaded by this block's flush
			std::lock_guard<std::mutex> lk(c->params_mu);
			c->h_blend[s] = gas_hrtf_blend{};
			mark_dirty(c->blend_dirty_flag, c->blend_dirty_list, s);
		}
		c->free_list.push_back(s);
		feed_drop(c, s); // ... nor a window row fed to the playback that is gone
		if (c->streams.h_cursors[s].pcm) {
			// a freed playback lets go of its stream (gas_stream_destroy must not see it as bound for ever, and a
			// re-allocated slot must not inherit the cursor): host mirror and device cursor both
			c->streams.h_cursors[s] = gas_cursor{};
			GAS_HIP(c, hipMemsetAsync(c->streams.d_cursors + s, 0, sizeof(gas_cursor), c->stream));
		}
	}
	c->pending_free.clear();
	c->cached_n = UINT32_MAX;
	return GAS_OK;
}

// HRTF sources take the frequency-domain path unless their peak is needed.
inline int launch_group(const gas_ctx *c, const SlotInfo &si, bool all_staged) {
	if (all_staged && si.kind == GAS_KIND_EFFECT && si.chain_sig != 0) {
		return G_FX_GENERIC;
	}
	const bool want_peak = wants_peak(c, si);
	if (si.group == G_FX_HRTF && want_peak && !uni_ok(c)) {
		return G_FX_HRTF_PK;
	}
	if (si.group == G_FX_ER_HRTF && want_peak) {
		return G_FX_ER_HRTF_PK;
	}
	return si.group;
}

// Validate + counting-sort the callback's slot list by launch group.  all_staged (gas_process_block_buses over effect
// kinds): every chain runs staged (rows out), the rows are mixed per bus.
int build_groups(gas_ctx *c, const uint32_t *slots, uint32_t n, bool all_staged) {
	uint32_t counts[G_COUNT] = { 0 };
	c->stamp.next();
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t s = slots[i];
		if (!live(c, s)) {
			return GAS_ERR_BAD_SLOT;
		}
		if (!c->slots[s].has_params) {
			return GAS_ERR_NO_PARAMS;
		}
		if (c->stamp.seen(s)) {
			return GAS_ERR_INVALID_ARGUMENT; // one playback twice in a callback would race on its state
		}
		counts[launch_group(c, c->slots[s], all_staged)]++;
	}
	uint32_t off = 0, cursor[G_COUNT];
	int nonempty = 0;
	for (int gt = 0; gt < G_COUNT; gt++) {
		c->groups[gt].offset = off;
		c->groups[gt].count = counts[gt];
		cursor[gt] = off;
		off += counts[gt];
		nonempty += counts[gt] > 0;
	}
	uint32_t *hs = c->h_idx, *hr = c->h_idx + c->cfg.max_sources;
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t p = cursor[launch_group(c, c->slots[slots[i]], all_staged)]++;
		hs[p] = slots[i];
		hr[p] = i;
	}
	c->chain_ranges.clear();
	if (c->groups[G_FX_GENERIC].count) { // runs of equal chains inside the staged group (stable: input order kept within a run)
		const Group &gg = c->groups[G_FX_GENERIC];
		std::vector<uint32_t> order(gg.count);
		for (uint32_t k = 0; k < gg.count; k++) {
			order[k] = k;
		}
		std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return c->slots[hs[gg.offset + a]].chain_sig < c->slots[hs[gg.offset + b]].chain_sig; });
		std::vector<uint32_t> ts(gg.count), tr(gg.count);
		for (uint32_t k = 0; k < gg.count; k++) {
			ts[k] = hs[gg.offset + order[k]];
			tr[k] = hr[gg.offset + order[k]];
		}
		for (uint32_t k = 0; k < gg.count; k++) {
			hs[gg.offset + k] = ts[k];
			hr[gg.offset + k] = tr[k];
			const uint32_t sig = c->slots[ts[k]].chain_sig;
			if (c->chain_ranges.empty() || c->chain_ranges.back().sig != sig) {
				ChainRange r;
				r.sig = sig;
				r.offset = k;
				c->chain_ranges.push_back(r);
			}
			c->chain_ranges.back().count++;
		}
	}
	for (int gt = 0; gt < G_COUNT; gt++) {
		Group &gr = c->groups[gt];
		gr.contiguous = gr.count > 0;
		gr.slot_base = gr.count ? hs[gr.offset] : 0;
		for (uint32_t k = 1; k < gr.count && gr.contiguous; k++) {
			gr.contiguous = hs[gr.offset + k] == gr.slot_base + k;
		}
	}
	c->cached_identity_rows = nonempty <= 1 && c->chain_ranges.size() <= 1;
	c->uni_peak_all = c->uni_peak_any = false;
	if (uni_ok(c) && c->groups[G_FX_HRTF].count > 0) {
		const Group &gh = c->groups[G_FX_HRTF];
		const uint32_t words = (gh.count + 31) / 32;
		std::memset(c->h_peak_bits, 0, (size_t)words * sizeof(uint32_t));
		uint32_t n_peak = 0;
		for (uint32_t k = 0; k < gh.count; k++) {
			if (wants_peak(c, c->slots[hs[gh.offset + k]])) {
				c->h_peak_bits[k >> 5] |= 1u << (k & 31);
				n_peak++;
			}
		}
		c->uni_peak_any = n_peak > 0;
		c->uni_peak_all = n_peak == gh.count;
		if (c->uni_peak_any && !c->uni_peak_all) {
			GAS_HIP(c, hipMemcpyAsync(c->d_peak_bits, c->h_peak_bits, (size_t)words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		}
	}
	// staged chains whose last stage is k_hrtf_uni: the same rule (an HRTF source that is not draining reports +inf)
	if (uni_ok(c) && (c->cfg.flags & GAS_FLAG_PEAKS_DRAINING_ONLY) != 0 && c->groups[G_FX_GENERIC].count > 0) {
		const Group &gg = c->groups[G_FX_GENERIC];
		const uint32_t half = (c->cfg.max_sources + 31) / 32, words = (gg.count + 31) / 32;
		uint32_t *bits = c->h_peak_bits + half;
		std::memset(bits, 0, (size_t)words * sizeof(uint32_t));
		bool partial = false;
		for (ChainRange &r : c->chain_ranges) {
			uint32_t n_peak = 0;
			for (uint32_t k = r.offset; k < r.offset + r.count; k++) {
				if (wants_peak(c, c->slots[hs[gg.offset + k]])) {
					bits[k >> 5] |= 1u << (k & 31);
					n_peak++;
				}
			}
			r.peak_any = n_peak > 0;
			r.peak_all = n_peak == r.count;
			partial = partial || (r.peak_any && !r.peak_all);
		}
		if (partial) {
			GAS_HIP(c, hipMemcpyAsync(c->d_peak_bits + half, bits, (size_t)words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		}
	}
	if (n > 0) {
		GAS_HIP(c, hipMemcpyAsync(c->d_slots, hs, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		if (!c->cached_identity_rows) {
			GAS_HIP(c, hipMemcpyAsync(c->d_rows, hr, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
			GAS_HIP(c, hipMemcpyAsync(c->d_slots_rows, slots, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		}
		GAS_HIP(c, hipStreamSynchronize(c->stream)); // h_idx is reused by the next list
	}
	c->cached_n = n;
	c->groups_gen++;
	return GAS_OK;
}

int needs_hrtf(const gas_ctx *c) {
	bool any = c->groups[G_FX_HRTF].count > 0 || c->groups[G_FX_ER_HRTF].count > 0 || c->groups[G_FX_HRTF_PK].count > 0 || c->groups[G_FX_ER_HRTF_PK].count > 0;
	for (const ChainRange &r : c->chain_ranges) {
		any = any || chain_has(r.sig, GAS_FX_HRTF);
	}
	return any && c->tab.spec == nullptr;
}

} // namespace

extern "C" {

int gas_abi_version(void) {
	return GAS_ABI_VERSION;
}

const char *gas_strerror(int status) {
	switch (status) {
		case GAS_OK:
			return "ok";
		case GAS_ERR_INVALID_ARGUMENT:
			return "invalid argument";
		case GAS_ERR_OUT_OF_SLOTS:
			return "no free source slot (max_sources reached)";
		case GAS_ERR_BAD_SLOT:
			return "slot is not allocated";
		case GAS_ERR_FRAME_COUNT:
			return "unexpected frame count (must equal the context's frames)";
		case GAS_ERR_NO_HRTF:
			return "an HRTF source was processed before gas_hrtf_load";
		case GAS_ERR_UNSUPPORTED_CHAIN:
			return "effect chain has no device kernel";
		case GAS_ERR_DEVICE:
			return "HIP runtime error (see gas_last_device_error)";
		case GAS_ERR_NO_DEVICE:
			return "no usable HIP device; this library has no CPU fallback";
		case GAS_ERR_OUT_OF_MEMORY:
			return "out of memory";
		case GAS_ERR_KIND_MISMATCH:
			return "operation does not apply to this source kind";
		case GAS_ERR_BAD_CHANNEL:
			return "unexpected channel";
		case GAS_ERR_NO_PARAMS:
			return "SpatializerParameters were never published for a source";
		default:
			return "unknown status";
	}
}

const char *gas_last_device_error(gas_ctx *ctx) {
	return ctx ? ctx->last_err.c_str() : "";
}

void gas_ctx_destroy(gas_ctx *c) {
	if (!c) {
		return;
	}
	(void)hipSetDevice(c->cfg.device);
	c->deferred.clear(); // callbacks still waiting for their batch are dropped with the context
	if (c->stream) {
		(void)hipStreamSynchronize(c->stream);
	}
	c->mem.release_all();
	if (c->own_stream && c->stream) {
		(void)hipStreamDestroy(c->stream);
	}
	delete c;
}

int gas_ctx_create(const gas_config *cfg, gas_ctx **out_ctx) {
	if (!cfg || !out_ctx || cfg->struct_size != sizeof(gas_config)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	*out_ctx = nullptr;
	if (cfg->max_sources == 0 || cfg->channel_count < 1 || cfg->channel_count > GAS_MAX_CHANNELS_PER_BUS || !(cfg->mix_rate > 0.0f)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (cfg->frames == 0 || cfg->frames > 512 || cfg->frames % 128 != 0) {
		return GAS_ERR_FRAME_COUNT;
	}
	if (cfg->er_ring_frames != 0 && ((cfg->er_ring_frames & (cfg->er_ring_frames - 1)) != 0 || cfg->er_ring_frames < 2 * cfg->frames)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if ((cfg->flags & GAS_FLAG_HRTF_INTERPOLATE) != 0 && (cfg->flags & (GAS_FLAG_HRTF_CROSSFADE | GAS_FLAG_DIRECTION_RUNS | GAS_FLAG_DIRECTION_ORDER | GAS_FLAG_XCD_ORDER)) != 0) {
		return GAS_ERR_INVALID_ARGUMENT; // those fade from, group by or order by a source's ONE direction
	}
	if ((cfg->flags & GAS_FLAG_HRTF_BLEND_FADE) != 0 && ((cfg->flags & GAS_FLAG_HRTF_INTERPOLATE) == 0 || (cfg->flags & (GAS_FLAG_HRTF_CROSSFADE | GAS_FLAG_DIRECTION_RUNS | GAS_FLAG_DIRECTION_ORDER | GAS_FLAG_XCD_ORDER)) != 0)) {
		return GAS_ERR_INVALID_ARGUMENT; // the fade is between blend rows: nothing to fade without them
	}
	if ((cfg->flags & GAS_FLAG_ER_TAP_FADE) != 0 && cfg->er_ring_frames == 0) {
		return GAS_ERR_INVALID_ARGUMENT; // the fade is between tap rows: no early-reflection stage without a ring
	}
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || cfg->device < 0 || cfg->device >= n_dev) {
		return GAS_ERR_NO_DEVICE;
	}
	gas_ctx *c = new (std::nothrow) gas_ctx();
	if (!c) {
		return GAS_ERR_OUT_OF_MEMORY;
	}
	c->cfg = *cfg;
	c->hist_len = 512 - cfg->frames / 2;
	c->sw = gas_switches_from_env();
	c->uni_er_enabled = c->sw.uni_er_mode != 0 && !er_fade_on(c); // the fused [ER, HRTF] kernels have no fading form: the tail of a staged chain stays two launches, whatever GAS_UNI_ER says
	const size_t N = cfg->max_sources;
	int rc = [&]() -> int {
		GAS_HIP(c, hipSetDevice(cfg->device));
		GAS_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
		c->own_stream = true;
		c->pipelined_mix = (cfg->flags & GAS_FLAG_PIPELINED_MIX) != 0;
		c->st.bq_stride = N * 8;
		GAS_HIP(c, device_zeroed(c, c->st.bq, GAS_BQ_FIELDS * c->st.bq_stride));
		GAS_HIP(c, device_zeroed(c, c->st.hrtf_hist, N * c->hist_len));
		GAS_HIP(c, device_zeroed(c, c->st.hrtf_prev_gain, N));
		GAS_HIP(c, device_zeroed(c, c->st.hrtf_prev_dir, N));
		if (cfg->er_ring_frames) {
			GAS_HIP(c, device_zeroed(c, c->st.er_ring, N * cfg->er_ring_frames));
			GAS_HIP(c, device_zeroed(c, c->st.er_pos, N));
		}
		GAS_HIP(c, device_zeroed(c, c->st.params, N));
		if ((cfg->flags & GAS_FLAG_HRTF_INTERPOLATE) != 0) { // every slot starts with the all-zero row: no blend
			GAS_HIP(c, device_zeroed(c, c->st.hrtf_blend, N));
		}
		if ((cfg->flags & GAS_FLAG_HRTF_BLEND_FADE) != 0) { // no slot has rendered yet: no old row to fade from
			GAS_HIP(c, device_zeroed(c, c->st.hrtf_prev_blend, N));
		}
		if (er_fade_on(c)) { // no slot has rendered yet: rendered == 0 everywhere
			GAS_HIP(c, device_zeroed(c, c->st.er_prev, N));
		}
		c->st.dyn_stride = (uint32_t)N;
		GAS_HIP(c, device_zeroed(c, c->st.dist_h, GAS_MAX_EFFECTS * 2 * N));
		GAS_HIP(c, device_zeroed(c, c->st.comp_rundb, GAS_MAX_EFFECTS * N));
		// the compressor's sidechain keys start silent
		GAS_HIP(c, device_zeroed(c, c->st.sidechain, GAS_MAX_SIDECHAINS * cfg->frames));
		GAS_HIP(c, c->mem.alloc(c->h_sidechain, GAS_MAX_SIDECHAINS * cfg->frames, Mem::PINNED));
		for (hipEvent_t &e : c->sidechain_ev) {
			GAS_HIP(c, c->mem.make_event(e, hipEventDisableTiming));
		}
		for (int f = 0; f < FX_FAMILIES; f++) { // the families that need no reservation for their settings: every slot starts from the engine's resource defaults
			if (k_fx_families[f].resident) {
				FxDev dev;
				const hipError_t e = fx_alloc_tables(c, f, dev, c->fx[f].h_settings);
				k_fx_families[f].set(c->st, dev);
				GAS_HIP(c, e);
				GAS_HIP(c, fx_alloc_upload(c, f, 0));
				c->fx[f].h_of.assign(N, fx_no_entries());
				c->fx[f].dirty_flag.assign(N, 0);
			}
		}
		GAS_HIP(c, c->mem.alloc(c->d_upload, N));
		GAS_HIP(c, c->mem.alloc(c->d_upload_slots, N));
		GAS_HIP(c, c->mem.alloc(c->d_slots, N));
		GAS_HIP(c, c->mem.alloc(c->d_rows, N));
		GAS_HIP(c, c->mem.alloc(c->d_slots_rows, N));
		GAS_HIP(c, c->mem.alloc(c->d_out, cfg->channel_count * cfg->frames));
		GAS_HIP(c, c->mem.alloc(c->d_peaks, 2 * N));
		GAS_HIP(c, c->mem.alloc(c->d_one_slot, 1));
		GAS_HIP(c, device_zeroed(c, c->st.was_further, N));
		GAS_HIP(c, device_zeroed(c, c->streams.d_cursors, N));
		GAS_HIP(c, c->mem.alloc(c->streams.d_slots, N));
		GAS_HIP(c, c->mem.alloc(c->streams.d_inc, N));
		GAS_HIP(c, c->mem.alloc(c->streams.h_inc, N, Mem::PINNED));
		c->feed.word.assign(N, GAS_FEED_NONE);
		{
			// end-of-stream ramp the stream-sampling prologue multiplies the last 64 valid frames by: tap k =
			// 0.96^(k+1) * (64 - k) / 64, the running f32 product and the f32 divide of audio_spatializer.cpp:382-392
			// (the host layer builds the same table for its CPU windows)
			constexpr int TAIL = GAS_LOOKAHEAD_BUFFER_SIZE;
			float env[TAIL];
			float decay = 1.0f;
			for (int k = 0; k < TAIL; k++) {
				decay *= 0.96f;
				env[k] = decay * ((float)TAIL - (float)k) / (float)TAIL;
			}
			GAS_HIP(c, c->mem.alloc(c->d_fade_env, TAIL));
			GAS_HIP(c, hipMemcpy(c->d_fade_env, env, sizeof(env), hipMemcpyHostToDevice));
		}
		GAS_HIP(c, c->mem.alloc(c->calc.d_cfgs, GAS_MAX_SPATIALIZER_CONFIGS));
		GAS_HIP(c, c->mem.alloc(c->calc.d_listeners, GAS_MAX_LISTENERS));
		GAS_HIP(c, c->mem.alloc(c->calc.d_slots, N));
		GAS_HIP(c, c->mem.alloc(c->calc.d_cfgidx, N));
		GAS_HIP(c, c->mem.alloc(c->h_params, N, Mem::PINNED));
		GAS_HIP(c, c->mem.alloc(c->h_upload, N, Mem::PINNED));
		GAS_HIP(c, c->mem.alloc(c->h_upload_slots, N, Mem::PINNED));
		GAS_HIP(c, c->mem.alloc(c->h_idx, 2 * N, Mem::PINNED));
		GAS_HIP(c, c->mem.alloc(c->h_peak_bits, 2 * ((N + 31) / 32), Mem::PINNED));
		GAS_HIP(c, c->mem.alloc(c->d_peak_bits, 2 * ((N + 31) / 32)));
		float2 h_tw[64 * 16];
		gas_make_twiddles(h_tw);
		GAS_HIP(c, c->mem.alloc(c->d_tw, 64 * 16));
		GAS_HIP(c, hipMemcpyAsync(c->d_tw, h_tw, sizeof(h_tw), hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, hipStreamSynchronize(c->stream));
		return GAS_OK;
	}();
	if (rc != GAS_OK) {
		gas_ctx_destroy(c);
		return rc;
	}
	c->slots.resize(N);
	c->h_routes.assign(N, gas_bus_route_default());
	c->streams.h_cursors.assign(N, gas_cursor{});
	c->stamp.at.assign(N, 0);
	c->calc.stamp.at.assign(N, 0);
	c->dirty_flag.assign(N, 0);
	if (blend_on(c)) {
		c->h_blend.assign(N, gas_hrtf_blend{});
		c->blend_dirty_flag.assign(N, 0);
	}
	c->free_list.reserve(N);
	for (size_t s = N; s-- > 0;) {
		c->free_list.push_back((uint32_t)s); // pop_back hands out 0, 1, 2, ...
	}
	*out_ctx = c;
	return GAS_OK;
}

int gas_ctx_set_stream(gas_ctx *c, void *hip_stream) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	{ // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
		const int rcd = flush_deferred(c);
		if (rcd != GAS_OK) {
			return rcd;
		}
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	{
		int rcj = join_outputs(c);
		if (rcj != GAS_OK) {
			return rcj;
		}
	}
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	if (c->own_stream) {
		GAS_HIP(c, hipStreamDestroy(c->stream));
		c->own_stream = false;
	}
	c->stream = reinterpret_cast<hipStream_t>(hip_stream);
	return GAS_OK;
}

int gas_ctx_get_config(gas_ctx *c, gas_config *out) {
	if (!c || !out) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	*out = c->cfg;
	return GAS_OK;
}

int gas_ctx_synchronize(gas_ctx *c) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	{ // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
		const int rcd = flush_deferred(c);
		if (rcd != GAS_OK) {
			return rcd;
		}
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	{
		int rcj = join_outputs(c);
		if (rcj != GAS_OK) {
			return rcj;
		}
	}
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	return GAS_OK;
}

int gas_ctx_set_batch_depth(gas_ctx *c, uint32_t depth) {
	if (!c || depth < 1 || depth > GAS_HRTF_MULTI_MAX_BLOCKS) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	{ // callbacks waiting for the old depth run first
		const int rcd = flush_deferred(c);
		if (rcd != GAS_OK) {
			return rcd;
		}
	}
	c->batch_depth = depth;
	return GAS_OK;
}

int gas_ctx_join_outputs(gas_ctx *c) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	{ // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
		const int rcd = flush_deferred(c);
		if (rcd != GAS_OK) {
			return rcd;
		}
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	return join_outputs(c);
}

int gas_source_alloc(gas_ctx *c, int kind, const int32_t *effects, uint32_t n_effects, uint32_t *out_slot) {
	if (!c || !out_slot || n_effects > GAS_MAX_EFFECTS || (n_effects > 0 && !effects)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	int g = group_of(kind, effects, n_effects);
	if (g == -1) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (g == -2) {
		return GAS_ERR_UNSUPPORTED_CHAIN;
	}
	if (g == G_FX_ER_HRTF && er_fade_on(c)) {
		g = G_FX_GENERIC; // GAS_FLAG_ER_TAP_FADE: the fused kernels do not fade; k_er_only<FADE> writes rows, the HRTF stage reads them
	}
	const uint32_t sig = (g == G_FX_GENERIC || (kind == GAS_KIND_EFFECT && n_effects > 0)) ? chain_signature(effects, n_effects) : 0; // fused chains keep theirs too: a bus callback runs them staged
	if ((g == G_FX_ER || g == G_FX_ER_HRTF || (g == G_FX_GENERIC && chain_has(sig, GAS_FX_EARLY_REFLECTIONS))) && c->cfg.er_ring_frames == 0) {
		return GAS_ERR_UNSUPPORTED_CHAIN;
	}
	uint32_t need[FX_FAMILIES][2] = {}; // pool entries of the chain, per family and pool
	bool in_family[FX_FAMILIES] = {}; // the chain has a kind whose settings the family carries
	for (int f = 0; f < FX_FAMILIES; f++) {
		for (uint32_t j = 0; j < n_effects; j++) {
			const int pool = k_fx_families[f].pool_of(effects[j]);
			if (pool >= 0) {
				need[f][pool]++;
			}
			in_family[f] = in_family[f] || k_fx_families[f].has_kind(effects[j]);
		}
	}
	std::lock_guard<std::mutex> alloc_lk(c->alloc_mu); // any thread (instantiate_playback_data runs on the physics thread, audio_spatializer.cpp:69)
	bool room = !c->free_list.empty();
	for (int f = 0; f < FX_FAMILIES; f++) {
		const FxFamily &p = c->fx[f];
		if (need[f][0] + need[f][1] > 0 && p.cap[0] == 0 && p.cap[1] == 0) {
			return GAS_ERR_UNSUPPORTED_CHAIN; // no pool reserved (gas_ctx_reserve_fx_*)
		}
		room = room && p.free[0].size() >= need[f][0] && p.free[1].size() >= need[f][1];
	}
	if (!room) { // all or nothing
		return GAS_ERR_OUT_OF_SLOTS;
	}
	const uint32_t s = c->free_list.back();
	if (c->slots[s].dirty_state) {
		GAS_HIP(c, hipSetDevice(c->cfg.device));
		GAS_HIP(c, gas_launch_zero_slot(c->stream, c->st, s, c->hist_len, c->cfg.er_ring_frames));
	}
	c->free_list.pop_back();
	SlotInfo si;
	si.used = 1;
	si.kind = (uint8_t)kind;
	si.group = (uint8_t)g;
	si.chain_sig = sig;
	c->slots[s] = si;
	*out_slot = s;
	for (int f = 0; f < FX_FAMILIES; f++) {
		if (in_family[f]) { // a new playback's effect instances start from the resource defaults (audio_spatializer_effect.cpp:79-88)
			fx_hand_out(c, f, s, effects, n_effects, sig);
		}
	}
	return GAS_OK;
}

int gas_source_free(gas_ctx *c, uint32_t slot) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	std::lock_guard<std::mutex> alloc_lk(c->alloc_mu); // any thread (a RefCounted destructor runs wherever the last reference drops)
	if (slot >= c->cfg.max_sources || !c->slots[slot].used || c->slots[slot].pending_free) {
		return GAS_ERR_BAD_SLOT;
	}
	// deferred like audio_spatializer.cpp:538-547: the audio thread may still name it this callback
	c->slots[slot].pending_free = 1;
	c->free_inbox.push_back(slot);
	return GAS_OK;
}

int gas_source_set_draining(gas_ctx *c, uint32_t slot, int draining) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (slot >= c->cfg.max_sources || !c->slots[slot].used) {
		return GAS_ERR_BAD_SLOT;
	}
	if (c->slots[slot].draining != (draining != 0)) {
		c->slots[slot].draining = draining != 0;
		c->cached_n = UINT32_MAX; // launch groups change: the next callback must pass its slot list again
	}
	return GAS_OK;
}

int gas_source_reset(gas_ctx *c, uint32_t slot) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	{ // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
		const int rcd = flush_deferred(c);
		if (rcd != GAS_OK) {
			return rcd;
		}
	}
	if (slot >= c->cfg.max_sources || !c->slots[slot].used) {
		return GAS_ERR_BAD_SLOT;
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	feed_drop(c, slot); // gas_source_feed_rows: a reset playback starts from silence
	GAS_HIP(c, gas_launch_zero_slot(c->stream, c->st, slot, c->hist_len, c->cfg.er_ring_frames));
	{ // its pool entries: zeroed by the next flush, before the next block (alloc_mu: the audio thread may be returning a
	  // freed slot's entries; the same lock order as gas_source_alloc)
		std::lock_guard<std::mutex> alloc_lk(c->alloc_mu);
		for (int f = 0; f < FX_FAMILIES; f++) {
			if (c->fx[f].cap[0] + c->fx[f].cap[1] > 0 && c->slots[slot].used) {
				std::lock_guard<std::mutex> lk(c->params_mu);
				fx_queue_zero(c, f, slot, c->slots[slot].chain_sig);
			}
		}
	}
	return GAS_OK;
}

int gas_params_publish(gas_ctx *c, uint32_t slot, const gas_params *params) {
	if (!c || !params) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (slot >= c->cfg.max_sources || !c->slots[slot].used) {
		return GAS_ERR_BAD_SLOT;
	}
	std::lock_guard<std::mutex> lk(c->params_mu);
	c->streams.params_touched = true;
	c->params_gen++;
	c->h_params[slot] = *params;
	mark_dirty(c->dirty_flag, c->dirty_list, slot);
	c->slots[slot].has_params = 1;
	return GAS_OK;
}

int gas_fx_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_settings *settings, uint32_t n) {
	return fx_publish(c, FX_BASIC, slots, settings, n);
}

int gas_hrtf_blend_publish(gas_ctx *c, const uint32_t *slots, const gas_hrtf_blend *blends, uint32_t n) {
	if (!c || !blend_on(c) || (n > 0 && (!slots || !blends))) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	const uint32_t dirs = c->tab.spec ? c->tab.dirs : 0; // no set loaded: the kernel clamps, as it clamps hrtf_dir
	for (uint32_t i = 0; i < n; i++) {
		if (slots[i] >= c->cfg.max_sources || !c->slots[slots[i]].used) {
			return GAS_ERR_BAD_SLOT;
		}
		for (int k = 0; k < 4; k++) {
			const float w = blends[i].weight[k];
			if (!std::isfinite(w) || w < 0.0f || (w != 0.0f && dirs != 0 && blends[i].dir[k] >= dirs)) {
				return GAS_ERR_INVALID_ARGUMENT;
			}
		}
	}
	std::lock_guard<std::mutex> lk(c->params_mu);
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t s = slots[i];
		c->h_blend[s] = blends[i];
		mark_dirty(c->blend_dirty_flag, c->blend_dirty_list, s);
	}
	return GAS_OK;
}

int gas_fx_dyn_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_dyn_settings *settings, uint32_t n) {
	return fx_publish(c, FX_DYN, slots, settings, n);
}

int gas_sidechain_set(gas_ctx *c, uint32_t key, const gas_audio_frame *frames, uint32_t frame_count, int mem) {
	if (!c || key >= GAS_MAX_SIDECHAINS || (mem != GAS_MEM_HOST && mem != GAS_MEM_DEVICE)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	const uint32_t F = c->cfg.frames;
	if (frame_count != F) {
		return GAS_ERR_FRAME_COUNT;
	}
	{ // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch detect on the blocks they were recorded behind
		const int rcd = flush_deferred(c);
		if (rcd != GAS_OK) {
			return rcd;
		}
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	const size_t bytes = (size_t)F * sizeof(gas_audio_frame);
	gas_audio_frame *dst = c->st.sidechain + (size_t)key * F;
	if (!frames) {
		GAS_HIP(c, hipMemsetAsync(dst, 0, bytes, c->stream));
		return GAS_OK;
	}
	if (mem == GAS_MEM_DEVICE) {
		const int rcj = join_outputs(c); // GAS_FLAG_PIPELINED_MIX: `frames` may be an earlier callback's out, still a pending sum
		if (rcj != GAS_OK) {
			return rcj;
		}
		GAS_HIP(c, hipMemcpyAsync(dst, frames, bytes, hipMemcpyDeviceToDevice, c->stream));
		return GAS_OK;
	}
	gas_audio_frame *stage = c->h_sidechain + (size_t)key * F;
	GAS_HIP(c, hipEventSynchronize(c->sidechain_ev[key])); // this key's previous upload has left the staging: a wait only while that upload is still queued (gas_amd.h)
	std::memcpy(stage, frames, bytes);
	GAS_HIP(c, hipMemcpyAsync(dst, stage, bytes, hipMemcpyHostToDevice, c->stream));
	GAS_HIP(c, hipEventRecord(c->sidechain_ev[key], c->stream));
	return GAS_OK;
}

int gas_fx_line_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_line_settings *settings, uint32_t n) {
	return fx_publish(c, FX_LINES, slots, settings, n);
}

int gas_ctx_reserve_fx_lines(gas_ctx *c, uint32_t delay_lines, uint32_t reverb_lines) {
	return fx_reserve(c, FX_LINES, delay_lines, reverb_lines);
}

int gas_fx_eq_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_eq_settings *settings, uint32_t n) {
	return fx_publish(c, FX_EQ, slots, settings, n);
}

int gas_ctx_reserve_fx_eq(gas_ctx *c, uint32_t eq_banks) {
	return fx_reserve(c, FX_EQ, eq_banks, 0);
}

int gas_fx_filter_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_filter_settings *settings, uint32_t n) {
	return fx_publish(c, FX_FILTER, slots, settings, n);
}

int gas_ctx_reserve_fx_filter(gas_ctx *c, uint32_t banks) {
	return fx_reserve(c, FX_FILTER, banks, 0);
}

int gas_fx_mod_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_mod_settings *settings, uint32_t n) {
	return fx_publish(c, FX_MOD, slots, settings, n);
}

int gas_ctx_reserve_fx_mod(gas_ctx *c, uint32_t chorus_lines, uint32_t phaser_banks) {
	return fx_reserve(c, FX_MOD, chorus_lines, phaser_banks);
}

int gas_fx_stereo_settings_publish(gas_ctx *c, const uint32_t *slots, const gas_fx_stereo_settings *settings, uint32_t n) {
	return fx_publish(c, FX_STEREO, slots, settings, n);
}

int gas_ctx_reserve_fx_stereo(gas_ctx *c, uint32_t enhance_rings) {
	return fx_reserve(c, FX_STEREO, enhance_rings, 0);
}

int gas_params_publish_batch(gas_ctx *c, const uint32_t *slots, const gas_params *params, uint32_t n, int params_mem) {
	if (!c || !params || (params_mem != GAS_MEM_HOST && params_mem != GAS_MEM_DEVICE)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (params_mem == GAS_MEM_HOST) {
		if (!slots) {
			return GAS_ERR_INVALID_ARGUMENT;
		}
		for (uint32_t i = 0; i < n; i++) {
			if (!live(c, slots[i])) {
				return GAS_ERR_BAD_SLOT;
			}
		}
		std::lock_guard<std::mutex> lk(c->params_mu);
		c->streams.params_touched = true;
		c->params_gen++;
		for (uint32_t i = 0; i < n; i++) {
			const uint32_t s = slots[i];
			c->h_params[s] = params[i];
			mark_dirty(c->dirty_flag, c->dirty_list, s);
			c->slots[s].has_params = 1;
		}
		return GAS_OK;
	}
	c->params_gen++;
	// Device-resident parameter rows (e.g. produced by a parameter kernel): scatter on the stream.
	// slots == NULL addresses the slot list of the last gas_process_block, in its row order.
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	if (slots) {
		GAS_TRY(flush_deferred(c)); // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
		GAS_TRY(flush_pending_params(c));
		if (n > c->cfg.max_sources) {
			return GAS_ERR_INVALID_ARGUMENT;
		}
		for (uint32_t i = 0; i < n; i++) {
			if (!live(c, slots[i])) {
				return GAS_ERR_BAD_SLOT;
			}
			c->slots[slots[i]].has_params = 1;
		}
		std::memcpy(c->h_upload_slots, slots, (size_t)n * sizeof(uint32_t));
		GAS_HIP(c, hipMemcpyAsync(c->d_upload_slots, c->h_upload_slots, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, gas_launch_scatter_params(c->stream, c->st.params, params, c->d_upload_slots, n));
		GAS_HIP(c, hipStreamSynchronize(c->stream));
	} else {
		if (c->cached_n != n) {
			return GAS_ERR_INVALID_ARGUMENT;
		}
		// Deferred: the next gas_process_block over this same list consumes the rows in its own launch when it can
		// (all sources [HRTF] or [ER, HRTF] chains), else scatters them first.  The buffer must stay untouched until then.
		if (c->pending_params) { // an earlier publish nobody consumed is about to be scattered: recorded callbacks first
			GAS_TRY(flush_deferred(c));
		}
		GAS_TRY(flush_pending_params(c));
		c->pending_params = params;
		c->pending_n = n;
	}
	return GAS_OK;
}

} // extern "C"

namespace gas_priv __attribute__((visibility("hidden"))) {
// Write the compact per-row mirror of the cached stream list back into the per-slot cursors.
void stream_rows_sync_back(gas_ctx *c) {
	for (size_t i = 0; i < c->streams.rows.size(); i++) {
		gas_cursor &cur = c->streams.h_cursors[c->streams.slots_host[i]];
		const StreamRow &r = c->streams.rows[i];
		if (cur.pcm) {
			cur.pos = r.looped ? r.pos : cur.frames - r.remaining;
		}
		if (r.resampled) {
			cur.fp_pos = r.fp_pos;
		}
		cur.has_frames = r.has_frames;
	}
	c->streams.rows.clear();
}
} // namespace gas_priv

namespace {
// The staging of the callback entries.  d_src holds at least `frames` frames afterwards.
// (hipFree synchronises the device by itself: waiting for the stream in front of it changes nothing observable.)
hipError_t ensure_src(gas_ctx *c, size_t frames) {
	if (frames <= c->d_src_frames) {
		return hipSuccess;
	}
	if (c->d_src) {
		(void)hipStreamSynchronize(c->stream);
	}
	return c->mem.grow(c->d_src, c->d_src_frames, frames ? frames : 1);
}

// Queues `out` and, when the caller wants them, the peaks of n sources back to the host, and waits for both.
hipError_t copy_back(gas_ctx *c, gas_audio_frame *out, const gas_audio_frame *d_out, size_t out_bytes, float *peaks, uint32_t n) {
	hipError_t e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess && peaks && n > 0) {
		e = hipMemcpyAsync(peaks, c->d_peaks, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
	}
	return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}

// A GAS_MEM_HOST callback runs on the library's own buffers; copy_back is the way home.  Makes room in d_src for the n
// rows and queues their upload (rows == nullptr: the rows are on the device already), and names what the launches
// write: d_out -- a bus callback: d_bus_out, allocated by the first call that needs it -- and d_peaks.
int stage_host(gas_ctx *c, const gas_audio_frame *rows, uint32_t n, bool buses, gas_audio_frame *&d_out, float *&d_peaks) {
	const size_t frames = (size_t)n * c->cfg.frames;
	if (rows) {
		GAS_HIP(c, ensure_src(c, frames));
		if (n > 0) {
			GAS_HIP(c, hipMemcpyAsync(c->d_src, rows, frames * sizeof(gas_audio_frame), hipMemcpyHostToDevice, c->stream));
		}
	}
	if (buses) {
		GAS_HIP(c, alloc_once(c, c->d_bus_out, (size_t)GAS_MAX_BUSES * c->cfg.channel_count * c->cfg.frames));
	}
	d_out = buses ? c->d_bus_out : c->d_out;
	d_peaks = c->d_peaks;
	return GAS_OK;
}

// What a bus callback can run: a list whose sources are all 3D mix (the empty list too), or all non-empty effect chains
// on a one-pair context -- plain [HRTF] every one of them, which has a fused form, or not.  Slots that are not live are
// skipped: build_groups rejects them.
enum BusList { BUS_LIST_NEITHER = 0, BUS_LIST_3D_MIX, BUS_LIST_CHAINS, BUS_LIST_PLAIN_HRTF };

BusList bus_list_form(const gas_ctx *c, const uint32_t *slots, uint32_t n) {
	bool all_mix = true, all_fx = n > 0, all_plain_hrtf = true;
	for (uint32_t i = 0; i < n; i++) {
		if (live(c, slots[i])) {
			const SlotInfo &si = c->slots[slots[i]];
			all_mix = all_mix && si.kind == GAS_KIND_3D_MIX;
			all_fx = all_fx && si.kind == GAS_KIND_EFFECT && si.chain_sig != 0;
			all_plain_hrtf = all_plain_hrtf && si.group == G_FX_HRTF;
		}
	}
	if (all_mix) {
		return BUS_LIST_3D_MIX;
	}
	if (!all_fx || c->cfg.channel_count != 1) {
		return BUS_LIST_NEITHER;
	}
	return all_plain_hrtf ? BUS_LIST_PLAIN_HRTF : BUS_LIST_CHAINS;
}
} // namespace

namespace gas_priv __attribute__((visibility("hidden"))) {
// The error exit of the callback entries.  Each entry's body returns its status, and the entry passes it through here
// once: a failed callback leaves a zeroed mix in host memory (the reference's ERR_FAIL paths,
// audio_spatializer.cpp:335-343); device memory is left as it is.  What an entry returns in FRONT of its body leaves
// `out` alone in both: the argument checks of every entry; in gas_process_block_buses the list reuse it cannot serve
// and the flush_deferred behind it; in the stream entries their flush_deferred -- and a bad n_buses there zeroes as
// much of a host `out` as a legal call could name.  gas_process_frames_1 / gas_mix_channel_1 never zero.
int fail_out(int code, int mem, gas_audio_frame *out, size_t out_bytes) {
	if (code != GAS_OK && mem == GAS_MEM_HOST) {
		std::memset(out, 0, out_bytes);
	}
	return code;
}
} // namespace gas_priv

namespace {

// What every callback body begins with: the caller's frame count is the context's, and the context's device is current.
int callback_begin(const gas_ctx *c, uint32_t frames) {
	if (frames != c->cfg.frames) {
		return GAS_ERR_FRAME_COUNT;
	}
	return hipSetDevice(c->cfg.device) == hipSuccess ? GAS_OK : GAS_ERR_NO_DEVICE;
}

// The body of gas_process_block behind its argument checks; a stream callback runs it with a fused source or with the
// rows it sampled (GAS_MEM_DEVICE).
int process_block(gas_ctx *c, const RowSource &src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, float *peaks, int mem) {
	const uint32_t F = c->cfg.frames, C = c->cfg.channel_count;
	GAS_TRY(callback_begin(c, frames));
	adopt_frees(c);
	if (!c->deferred.empty()) { // GAS_FLAG_BATCHED_LAUNCH: do the waiting callbacks still see what they were recorded with?
		bool host_dirty = false;
		{
			std::lock_guard<std::mutex> lk(c->params_mu);
			host_dirty = !c->dirty_list.empty() || !c->fx[FX_BASIC].dirty_list.empty() || !c->blend_dirty_list.empty();
		}
		const bool keep = mem == GAS_MEM_DEVICE && !slots && n == c->deferred_n && c->pending_free.empty() && c->groups_gen == c->deferred_groups_gen && !host_dirty;
		if (!keep) {
			GAS_TRY(flush_deferred(c));
		}
	}
	if (c->pending_params && (slots || n == 0 || c->cached_n != n || !c->pending_free.empty())) {
		GAS_TRY(flush_pending_params(c)); // the list may change: scatter with the mapping it was published for
	}
	apply_pending_frees(c);
	if (slots || n == 0) { // an empty callback needs no list
		c->cached_n = UINT32_MAX; // what a list that build_groups rejects leaves behind
		GAS_TRY(build_groups(c, slots, n, false));
	} else if (c->cached_n != n) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (needs_hrtf(c)) {
		return GAS_ERR_NO_HRTF;
	}
	const uint64_t pgen = c->params_gen.load(); // read before the snapshot: a publish racing with it re-sorts next time
	GAS_TRY(flush_params(c)); // one snapshot per callback (audio_spatializer.cpp:328)
	if (c->order_groups_gen != c->groups_gen || c->order_params_gen != pgen) {
		std::memset(c->order_ok, 0, sizeof(c->order_ok));
		c->order_groups_gen = c->groups_gen;
		c->order_params_gen = pgen;
	}

	RowSource d_src = src;
	gas_audio_frame *d_out = out;
	float *d_peaks = peaks ? peaks : c->d_peaks;
	if (mem == GAS_MEM_HOST) {
		GAS_TRY(stage_host(c, src.rows, n, false, d_out, d_peaks));
		d_src.rows = c->d_src;
	}
	const gas_params *fresh = nullptr; // device-published rows this callback's HRTF launch reads itself
	if (c->pending_params) {
		bool only_hrtf = true;
		for (int gt = 0; gt < G_COUNT; gt++) {
			only_hrtf = only_hrtf && (gt == G_FX_HRTF || gt == G_FX_HRTF_PK || gt == G_FX_ER_HRTF || gt == G_FX_ER_HRTF_PK || c->groups[gt].count == 0);
		}
		if (only_hrtf && c->pending_n == n) {
			fresh = c->pending_params; // k_hrtf_ols reads the rows and writes them through
			c->pending_params = nullptr;
		} else {
			GAS_TRY(flush_pending_params(c));
		}
	}
	if (mem == GAS_MEM_DEVICE && batchable(c, n, src.fused())) {
		gas_ctx::Deferred cur;
		cur.src = d_src.rows;
		cur.out = d_out;
		cur.peaks = d_peaks;
		cur.fresh = fresh;
		c->deferred.push_back(cur); // nothing is enqueued yet: this callback runs with its neighbours (or when flushed)
		c->deferred_n = n;
		c->deferred_groups_gen = c->groups_gen;
		const uint32_t depth = c->batch_depth < GAS_HRTF_MULTI_MAX_BLOCKS ? c->batch_depth : GAS_HRTF_MULTI_MAX_BLOCKS;
		return c->deferred.size() >= depth ? flush_deferred(c) : GAS_OK;
	}
	GAS_TRY(flush_deferred(c));
	RunArgs a = own_list(c, d_src, n, d_out, d_peaks);
	a.channel_count = C;
	a.use_order = true;
	a.pipelined = mem == GAS_MEM_DEVICE;
	a.fresh = fresh;
	GAS_TRY(run_groups(c, a));
	if (mem == GAS_MEM_HOST) {
		GAS_HIP(c, copy_back(c, out, c->d_out, (size_t)C * F * sizeof(gas_audio_frame), peaks, n));
	}
	return GAS_OK;
}

// The routes snapshot of a bus callback (latest wins), like the parameters.
int flush_routes(gas_ctx *c) {
	bool upload = false;
	{
		std::lock_guard<std::mutex> lk(c->params_mu);
		if (c->routes_dirty || !c->d_routes) {
			GAS_HIP(c, alloc_once(c, c->h_routes_pinned, c->cfg.max_sources, Mem::PINNED));
			GAS_HIP(c, alloc_once(c, c->d_routes, c->cfg.max_sources));
			std::memcpy(c->h_routes_pinned, c->h_routes.data(), sizeof(gas_bus_route) * c->cfg.max_sources);
			c->routes_dirty = false;
			upload = true;
		}
	}
	if (upload) {
		GAS_HIP(c, hipMemcpyAsync(c->d_routes, c->h_routes_pinned, sizeof(gas_bus_route) * c->cfg.max_sources, hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, hipStreamSynchronize(c->stream)); // the pinned mirror is rewritten by the next snapshot
	}
	return GAS_OK;
}

// The body of process_block_buses.  AudioSpatializer3D's buses in one launch: the mix_channel kernel with per-source
// weights per bus, its partial planes summed by the ordinary deterministic reduce (bus-major: plane b * C + c).
int bus_body(gas_ctx *c, const RowSource &src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, uint32_t n_buses, float *peaks, int mem) {
	const uint32_t F = c->cfg.frames, C = c->cfg.channel_count;
	GAS_TRY(callback_begin(c, frames));
	GAS_TRY(flush_pending_params(c));
	apply_pending_frees(c);
	// Two forms: every source GAS_KIND_3D_MIX (the mix-channel buses of AudioSpatializer3D, fused in the biquad
	// kernels), or every source an effect chain (run staged: per-source rows, then mixed per bus) on a one-pair context.
	const bool reuse = n > 0 && !slots; // the cached form is 1 (3D mix) or 2 (fused [HRTF]) then
	const BusList form = reuse ? (c->bus_form_cached == 1 ? BUS_LIST_3D_MIX : BUS_LIST_PLAIN_HRTF) : bus_list_form(c, slots, n);
	// [HRTF] sources onto one or two buses have a fused form (k_hrtf_uni<BUS2>: the second bus's spectra sums in LDS)
	// (three to six buses: one fused launch per pair of buses, the state committed by the last)
	const bool fused_hrtf = form == BUS_LIST_PLAIN_HRTF && uni_ok(c) && gas_hrtf_uni_waves() == 8;
	if (src.fused() && !(fused_hrtf && mem == GAS_MEM_DEVICE)) {
		return GAS_ERR_INVALID_ARGUMENT; // gas_process_block_streams_buses hands over no rows: only the fused form can sample
	}
	const bool staged = (form == BUS_LIST_CHAINS || form == BUS_LIST_PLAIN_HRTF) && !fused_hrtf;
	if (reuse && staged) {
		return GAS_ERR_INVALID_ARGUMENT; // the staged form regroups: it needs the list
	}
	if (!reuse) {
		c->cached_n = UINT32_MAX; // what a list that build_groups rejects leaves behind
		GAS_TRY(build_groups(c, slots, n, staged));
		if (staged) {
			c->cached_n = UINT32_MAX; // the staged grouping is this call's only: a later list reuse must regroup
		}
	}
	c->bus_form_cached = staged ? 0 : (fused_hrtf ? 2 : (form == BUS_LIST_3D_MIX ? 1 : 0));
	c->bus_form_groups_gen = c->groups_gen;
	for (int gt = 0; gt < G_COUNT; gt++) {
		if (gt != (staged ? G_FX_GENERIC : (fused_hrtf ? G_FX_HRTF : G_3D_MIX)) && c->groups[gt].count > 0) {
			c->cached_n = UINT32_MAX;
			return GAS_ERR_UNSUPPORTED_CHAIN;
		}
	}
	if ((staged || fused_hrtf) && needs_hrtf(c)) {
		return GAS_ERR_NO_HRTF;
	}
	GAS_TRY(join_outputs(c));
	GAS_TRY(flush_params(c));
	GAS_TRY(flush_routes(c));
	const uint32_t P = n ? (fused_hrtf ? gas_hrtf_uni_partials(n) : gas_biquad_partials(n)) : 0;
	const size_t need = (size_t)(fused_hrtf ? 2 * ((n_buses + 1) / 2) : n_buses) * C * (P ? P : 1) * F * 2; // the fused [HRTF] form writes two planes per launch
	if (need > c->bus_partial_floats) {
		GAS_HIP(c, hipStreamSynchronize(c->stream));
		GAS_HIP(c, c->mem.grow(c->d_bus_partials, c->bus_partial_floats, need));
	}
	RowSource d_src = src;
	gas_audio_frame *d_out = out;
	float *d_peaks = peaks ? peaks : c->d_peaks;
	if (mem == GAS_MEM_HOST) {
		GAS_TRY(stage_host(c, src.rows, n, true, d_out, d_peaks));
		d_src.rows = c->d_src;
	}
	if (fused_hrtf && n > 0) {
		// bus b's partial rows: [b * P, (b + 1) * P); one launch per pair of buses, the last one commits the state
		gas_hrtf_uni_launch lu = plain_uni_launch(c, own_hrtf_group(c, d_src.rows, n, d_peaks), d_src, c->d_bus_partials, 0);
		lu.routes = c->d_routes;
		lu.bus_rows = P;
		const uint32_t passes = (n_buses + 1) / 2;
		for (uint32_t pass = 0; pass < passes; pass++) {
			lu.p_offset = 2 * pass * P;
			lu.bus_base = 2 * pass;
			lu.commit = pass + 1 == passes;
			GAS_HIP(c, gas_launch_hrtf_uni(lu));
		}
	} else if (staged) {
		// effect kinds: the stages of every chain with rows out, then k_rows_accumulate_buses and one reduce over the
		// buses (run_groups' staged-chain path, told about the buses)
		gas_bus_args ba;
		ba.routes = c->d_routes;
		ba.n_buses = n_buses;
		RunArgs a = own_list(c, d_src, n, d_out, d_peaks);
		a.buses = &ba;
		GAS_TRY(run_groups(c, a));
	} else if (n > 0) {
		GAS_HIP(c, hipMemsetAsync(d_peaks, 0, (size_t)n * 2 * sizeof(float), c->stream)); // k_biquad_mix accumulates peaks over channel pairs
		gas_group_args ga;
		ga.src = d_src.rows;
		ga.rows = c->cached_identity_rows ? nullptr : c->d_rows;
		ga.slots = c->d_slots;
		ga.slot_base = 0;
		ga.n = n;
		ga.peaks = d_peaks;
		gas_bus_args ba;
		ba.routes = c->d_routes;
		ba.n_buses = n_buses;
		// force the multi-bus code even for one bus when the caller routes (a lone bus other than 0 is legal)
		gas_biquad_launch lb = biquad_launch(c, GAS_MODE_MIX_CHANNEL, ga, c->d_bus_partials, 0);
		lb.channel_count = C;
		lb.p_stride = P;
		lb.buses = ba;
		GAS_HIP(c, gas_launch_biquad_mix(lb));
	}
	if (!staged) {
		GAS_HIP(c, gas_launch_mix_reduce(c->stream, c->d_bus_partials, P, P ? P : 1, n_buses * C, F, d_out));
	}
	if (mem == GAS_MEM_HOST) {
		GAS_HIP(c, copy_back(c, out, c->d_bus_out, (size_t)n_buses * C * F * sizeof(gas_audio_frame), peaks, n));
	}
	return GAS_OK;
}

// gas_process_block_buses behind its argument checks; a stream callback runs it with a fused source or with the rows
// it sampled (GAS_MEM_DEVICE).  slots == NULL: the list (and grouping) of the previous call, like gas_process_block --
// for the two forms whose grouping is the ordinary one (3D mix, fused [HRTF]).
int process_block_buses(gas_ctx *c, const RowSource &src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, uint32_t n_buses, float *peaks, int mem) {
	adopt_frees(c);
	if (n > 0 && !slots && (c->cached_n != n || c->bus_form_cached == 0 || c->bus_form_groups_gen != c->groups_gen || !c->pending_free.empty())) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	GAS_TRY(flush_deferred(c)); // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
	return fail_out(bus_body(c, src, slots, n, frames, out, n_buses, peaks, mem), mem, out, (size_t)n_buses * c->cfg.channel_count * c->cfg.frames * sizeof(gas_audio_frame));
}

// The body of gas_process_frames_1 and gas_mix_channel_1 (host memory).  No exit of it touches `out`.
int process_one(gas_ctx *c, uint32_t slot, int channel, bool mix_channel, gas_audio_frame *out, const gas_audio_frame *src, int frame_count) {
	if (!c || !out || !src) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	GAS_TRY(flush_deferred(c)); // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
	const uint32_t F = c->cfg.frames;
	if (frame_count < 0 || (uint32_t)frame_count != F) {
		return GAS_ERR_FRAME_COUNT;
	}
	if (!live(c, slot)) {
		return GAS_ERR_BAD_SLOT;
	}
	const SlotInfo &si = c->slots[slot];
	if (!si.has_params) {
		return GAS_ERR_NO_PARAMS;
	}
	const bool is3d = si.kind == GAS_KIND_3D_MIX || si.kind == GAS_KIND_3D_PROCESS;
	if (mix_channel) {
		if (!is3d) {
			return GAS_ERR_KIND_MISMATCH;
		}
		if (channel < 0 || channel >= GAS_MAX_CHANNELS_PER_BUS) { // ERR_FAIL_INDEX_V(p_channel, 4, nullptr), audio_spatializer_3d.cpp:888
			return GAS_ERR_BAD_CHANNEL;
		}
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	Group groups[G_COUNT];
	int gt = si.group;
	int force_mode = -1;
	if (is3d) {
		gt = G_3D_MIX;
		force_mode = mix_channel ? GAS_MODE_MIX_CHANNEL : GAS_MODE_PROCESS_FRAMES;
	}
	if (gt == G_FX_HRTF) {
		gt = G_FX_HRTF_PK;
	} else if (gt == G_FX_ER_HRTF) {
		gt = G_FX_ER_HRTF_PK;
	}
	groups[gt].offset = 0;
	groups[gt].count = 1;
	if ((gt == G_FX_HRTF_PK || gt == G_FX_ER_HRTF_PK) && c->tab.spec == nullptr) {
		return GAS_ERR_NO_HRTF;
	}
	GAS_TRY(flush_pending_params(c));
	GAS_TRY(flush_params(c));
	gas_audio_frame *d_out = nullptr;
	float *d_peaks = nullptr;
	GAS_TRY(stage_host(c, src, 1, false, d_out, d_peaks));
	GAS_HIP(c, hipMemcpyAsync(c->d_one_slot, &slot, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	std::vector<ChainRange> one_range;
	if (gt == G_FX_GENERIC) {
		ChainRange r;
		r.sig = si.chain_sig;
		r.count = 1;
		one_range.push_back(r);
		if (chain_has(r.sig, GAS_FX_HRTF) && c->tab.spec == nullptr) {
			return GAS_ERR_NO_HRTF;
		}
	}
	RunArgs a;
	a.src.rows = c->d_src;
	a.slots = c->d_one_slot;
	a.groups = groups;
	a.ranges = &one_range;
	a.n_total = 1;
	a.out = d_out;
	a.peaks = d_peaks;
	a.channel_begin = mix_channel ? (uint32_t)channel : 0;
	a.force_mode = force_mode;
	GAS_TRY(run_groups(c, a));
	GAS_HIP(c, copy_back(c, out, d_out, (size_t)F * sizeof(gas_audio_frame), nullptr, 0));
	return GAS_OK;
}

// The stream callback, step by step.  Is this the list of the previous stream callback, its launch groups still cached, and no parameter or binding
// change since?  Then the callback skips validation and works on the compact row mirror.
bool stream_list_unchanged(const gas_ctx *c, const uint32_t *slots, uint32_t n, bool buses) {
	const StreamState &s = c->streams;
	return c->pending_free.empty() // a deferred free re-sorts the groups
			&& s.rows.size() == n
			&& (c->cached_n == n || (buses && s.bus_staged)) // the staged bus form regroups on every call and leaves no cached groups behind: its list stays "the same" without them
			&& s.last_buses == buses
			&& s.groups_gen == c->groups_gen
			&& !s.params_touched
			&& s.slots_host.size() == n
			&& (n == 0 || std::memcmp(s.slots_host.data(), slots, (size_t)n * sizeof(uint32_t)) == 0);
}

// A new list: folds the old row mirror back into the cursors, checks the list, rebuilds the mirror and the list's
// traits from the cursors, and uploads the slots and the resampled playbacks' steps.  Everything the callback can
// reject its list for is checked BEFORE a cursor moves: the reference consumes a playback's frames only when it mixes
// them (audio_spatializer.cpp:378), so a failed callback must leave the playback cursors (host mirror and device)
// where they were.
int stream_list_adopt(gas_ctx *c, const uint32_t *slots, uint32_t n, bool buses) {
	StreamState &s = c->streams;
	stream_rows_sync_back(c);
	for (uint32_t i = 0; i < n; i++) {
		if (!live(c, slots[i])) {
			return GAS_ERR_BAD_SLOT;
		}
		const float pitch = c->slots[slots[i]].has_params ? c->h_params[slots[i]].pitch_scale : 1.0f;
		if (!s.h_cursors[slots[i]].pcm) {
			// bound to no stream: a fed row or silence.  pitch_scale is the sampler's input, and whoever decodes this
			// playback has applied it already (the host layer hands it to the playback's mix callback), as for the
			// rows of gas_process_block
		} else if (s.h_cursors[slots[i]].resampled) {
			if (!(pitch >= 0.0f && pitch < 32768.0f)) {
				return GAS_ERR_INVALID_ARGUMENT;
			}
		} else if (pitch != 1.0f && pitch != 0.0f) {
			return GAS_ERR_UNSUPPORTED_CHAIN; // a non-resampled playback class (gas_stream_set_resampled is off)
		}
	}
	// what gas_process_block could still reject
	c->stamp.next();
	for (uint32_t i = 0; i < n; i++) {
		const SlotInfo &si = c->slots[slots[i]];
		if (!si.has_params) {
			return GAS_ERR_NO_PARAMS;
		}
		if (c->stamp.seen(slots[i])) {
			return GAS_ERR_INVALID_ARGUMENT; // one playback twice in a callback
		}
		const bool wants_hrtf = si.group == G_FX_HRTF || si.group == G_FX_ER_HRTF || (si.group == G_FX_GENERIC && chain_has(si.chain_sig, GAS_FX_HRTF));
		if (wants_hrtf && c->tab.spec == nullptr) {
			return GAS_ERR_NO_HRTF;
		}
	}
	if (buses && bus_list_form(c, slots, n) == BUS_LIST_NEITHER) {
		return GAS_ERR_UNSUPPORTED_CHAIN; // process_block_buses would, after the cursors have moved
	}
	s.last_buses = buses;
	s.bus_staged = false;
	s.params_touched = false;
	s.slots_host.assign(slots, slots + n);
	s.rows.resize(n);
	s.list = StreamListTraits{};
	s.list.all_hrtf = n > 0;
	for (uint32_t i = 0; i < n; i++) {
		const gas_cursor &cur = s.h_cursors[slots[i]];
		s.list.any_adpcm = s.list.any_adpcm || (cur.pcm && (cur.format_channels >> 8) == GAS_PCM_IMA_ADPCM);
		s.list.any_qoa = s.list.any_qoa || (cur.pcm && (cur.format_channels >> 8) == GAS_PCM_QOA);
		StreamRow &r = s.rows[i];
		r.remaining = cur.pcm && cur.frames > cur.pos ? cur.frames - cur.pos : 0;
		r.has_frames = cur.pcm ? cur.has_frames : 0;
		r.resampled = cur.pcm ? cur.resampled : 0;
		r.looped = cur.pcm && cur.loop_mode ? 1 : 0;
		r.pos = cur.pos;
		s.list.any_looped = s.list.any_looped || r.looped;
		r.inc = 65536;
		if (r.resampled) {
			// [ENGINE] mix_increment = uint64((stream_rate * rate_scale / mix_rate) * FP_LEN), stream at the mix rate
			const float pitch = c->slots[slots[i]].has_params ? c->h_params[slots[i]].pitch_scale : 1.0f;
			r.inc = (uint32_t)(uint64_t)(((double)(c->cfg.mix_rate * pitch) / (double)c->cfg.mix_rate) * 65536.0);
			r.fp_pos = cur.fp_pos;
			r.end_fp = cur.frames << 16;
			s.list.any_resampled = true;
		}
		s.h_inc[i] = r.inc;
		s.list.all_hrtf = s.list.all_hrtf && c->slots[slots[i]].group == G_FX_HRTF;
	}
	if (s.list.any_resampled) {
		GAS_HIP(c, hipMemcpyAsync(s.d_inc, s.h_inc, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, hipStreamSynchronize(c->stream)); // the pinned staging array is rewritten by the next list
	}
	if (n > 0) {
		GAS_HIP(c, hipMemcpyAsync(s.d_slots, s.slots_host.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	}
	return GAS_OK;
}

// One row's share of a callback of F frames: the same arithmetic as k_sample_sources.  (Inlined into stream_advance's
// loop: no call per row.)
inline void stream_row_advance(StreamRow &r, uint32_t F) {
	if (r.has_frames && r.resampled) { // k_sample_sources' resampled branch
		uint64_t mixed = F;
		if (r.looped) {
			// never runs out
		} else if (r.fp_pos >= r.end_fp) {
			mixed = 0;
		} else if (r.inc > 0) {
			const uint64_t need = (r.end_fp - r.fp_pos + r.inc - 1) / r.inc;
			mixed = need < F ? need : F;
		}
		r.fp_pos += (uint64_t)F * r.inc;
		if (mixed != F) {
			r.has_frames = 0;
		}
	} else if (r.has_frames && r.looped) {
		r.pos += F;
	} else if (r.has_frames) {
		const uint32_t mixed = r.remaining < F ? (uint32_t)r.remaining : F;
		r.remaining -= mixed;
		if (mixed != F) {
			r.has_frames = 0;
		}
	}
}

// The host mirror of one callback's cursor arithmetic: which playbacks end inside this callback
// (audio_spatializer.cpp:380,398), the caller's has_frames, the draining marks, and the feed words.  Which entries take
// a fed row is this callback's matter alone, read from the pending rows and never from the cached list -- the steady
// state holds whatever is fed, not fed, or fed again under it.  Sets draining_changed when a playback that ended makes
// its slot draining (the launch groups must be rebuilt), any_fed when an entry takes a fed row (feed.entry holds this
// callback's words).  One loop over the rows: in the steady state it is the host cost of a stream callback.
void stream_advance(gas_ctx *c, const uint32_t *slots, uint32_t n, uint8_t *has_frames, bool &draining_changed, bool &any_fed) {
	FeedState &f = c->feed;
	const uint32_t F = c->cfg.frames;
	const bool feed_pending = !f.slots.empty();
	if (feed_pending) {
		f.entry.assign(n, GAS_FEED_NONE);
	}
	for (uint32_t i = 0; i < n; i++) {
		StreamRow &r = c->streams.rows[i];
		if (feed_pending && f.word[slots[i]] != GAS_FEED_NONE) { // a live playback without a cursor: nothing moves, nothing ends
			f.entry[i] = f.word[slots[i]];
			any_fed = true;
			r.draining_marked = 0; // the next callback that finds it unfed marks it draining again
			if (has_frames) {
				has_frames[i] = 1;
			}
			continue;
		}
		stream_row_advance(r, F);
		if (!r.has_frames && !r.draining_marked) {
			r.draining_marked = 1;
			if (!c->slots[slots[i]].draining) {
				c->slots[slots[i]].draining = 1; // from now on the gate reads its peak (:464)
				draining_changed = true;
			}
		}
		if (has_frames) {
			has_frames[i] = (uint8_t)r.has_frames;
		}
	}
}

// The feed table's header follows the list and the fed set: uploads this callback's words when they differ from the
// words it holds.  Then the pending rows are spent -- one feed serves one callback; rows of slots the list does not
// name go with it.  (A failed upload spends nothing.)
int feed_serve(gas_ctx *c, uint32_t n, bool any_fed) {
	FeedState &f = c->feed;
	if (any_fed && f.entry != f.entry_dev) {
		f.entry_dev.clear(); // until the upload is queued the header counts as unknown
		GAS_HIP(c, hipEventSynchronize(f.entry_ev)); // the previous header has left the pinned words: a wait only while that upload is still queued
		std::memcpy(f.h_entry, f.entry.data(), (size_t)n * sizeof(uint32_t));
		GAS_HIP(c, hipMemcpyAsync(f.d_table, f.h_entry, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, hipEventRecord(f.entry_ev, c->stream));
		f.entry_dev = f.entry;
	}
	if (!f.slots.empty()) {
		for (uint32_t s : f.slots) {
			f.word[s] = GAS_FEED_NONE;
		}
		f.slots.clear();
		f.used = 0;
	}
	return GAS_OK;
}

// May the HRTF launch sample the list's windows itself (k_hrtf_ols / k_hrtf_uni<SRC_PCM>), so that no rows are staged?
bool stream_fuses(const gas_ctx *c, bool buses, bool any_fed) {
	const StreamListTraits &l = c->streams.list;
	// the fused prologues sample plain playbacks only: every chain a plain [HRTF], every stream uncompressed and at the
	// mix rate (a resampled, GAS_PCM_IMA_ADPCM or GAS_PCM_QOA playback samples rows first)
	const bool plain = l.all_hrtf && !l.any_resampled && !l.any_adpcm && !l.any_qoa;
	// GAS_FLAG_HRTF_BLEND_FADE: the stream-sampling form has no registers left for the fade
	const bool fade_free = !fade_on(c);
	// gas_stream_set_loop: the cross-fade form has no registers left for the looped branch either
	const bool loops_fused = !l.any_looped || (c->cfg.flags & GAS_FLAG_HRTF_CROSSFADE) == 0;
	// buses: the fused form is k_hrtf_uni<SRC_PCM, BUS2>, which gas_process_block_buses picks on a one-pair context without a k_hrtf_ols-only mode
	const bool bus_fusable = !buses || (c->cfg.channel_count == 1 && uni_ok(c) && gas_hrtf_uni_waves() == 8);
	// gas_source_feed_rows: k_hrtf_uni<SRC_PCM> and k_hrtf_uni<SRC_PCM, BUS2> take fed entries; the k_hrtf_ols stream-sampling forms -- cross-fade, direction runs / order, interpolation contexts -- have no registers left for them
	const bool fed_fusable = !any_fed || uni_ok(c);
	return plain && fade_free && loops_fused && !c->sw.rows_first && bus_fusable && fed_fusable;
}

// Rows first: the windows of the list's n playbacks into d_src -- k_sample_sources, then the decoders of the compressed
// streams the list holds.
int stream_sample_rows(gas_ctx *c, uint32_t n, const uint8_t *feed) {
	const StreamState &s = c->streams;
	const uint32_t F = c->cfg.frames;
	if (ensure_src(c, (size_t)n * F) != hipSuccess) {
		return GAS_ERR_OUT_OF_MEMORY;
	}
	if (n == 0) {
		return GAS_OK;
	}
	const uint32_t *inc = s.list.any_resampled ? s.d_inc : nullptr;
	GAS_HIP(c, gas_launch_sample_sources(c->stream, s.d_cursors, s.d_slots, n, F, c->d_fade_env, c->d_src, inc, feed));
	if (s.list.any_adpcm) {
		GAS_HIP(c, gas_launch_sample_adpcm(c->stream, s.d_cursors, s.d_slots, n, F, c->d_fade_env, c->d_src, inc, c->sw.adpcm_span));
	}
	if (s.list.any_qoa) {
		GAS_HIP(c, gas_launch_sample_qoa(c->stream, s.d_cursors, s.d_slots, n, F, c->d_fade_env, c->d_src, inc, c->sw.qoa_span));
	}
	return GAS_OK;
}

// The body of both stream entries: the steps above, then gas_process_block[_buses]' device path over the windows (a
// host `out`: into the library's buffers, one copy back).
int stream_body(gas_ctx *c, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, size_t out_bytes, uint32_t n_buses, bool buses, float *peaks, uint8_t *has_frames, int mem) {
	const uint32_t F = c->cfg.frames;
	GAS_TRY(callback_begin(c, frames));
	adopt_frees(c);
	bool same_list = stream_list_unchanged(c, slots, n, buses);
	if (!same_list) {
		GAS_TRY(stream_list_adopt(c, slots, n, buses));
	}
	bool draining_changed = false, any_fed = false;
	stream_advance(c, slots, n, has_frames, draining_changed, any_fed);
	if (draining_changed) {
		c->cached_n = UINT32_MAX;
		same_list = false;
	}
	GAS_TRY(feed_serve(c, n, any_fed));
	const uint8_t *feed = any_fed ? c->feed.d_table : nullptr;
	const bool fused = c->streams.last_fused = stream_fuses(c, buses, any_fed);
	RowSource rows;
	if (fused) { // no float rows: the HRTF launch samples the bound streams (and the fed rows) itself
		rows.cursors = c->streams.d_cursors;
		rows.feed = feed;
	} else {
		GAS_TRY(stream_sample_rows(c, n, feed));
		rows.rows = c->d_src;
	}
	gas_audio_frame *d_out = out;
	float *d_pk = peaks;
	if (mem == GAS_MEM_HOST) {
		GAS_TRY(stage_host(c, nullptr, n, buses, d_out, d_pk));
	}
	int rc = GAS_OK;
	if (buses) {
		// gas_process_block_buses reuses a list only for its 3D-mix and fused [HRTF] forms; the staged form needs it every time
		const bool reuse = same_list && n > 0 && c->cached_n == n && c->bus_form_cached != 0 && c->bus_form_groups_gen == c->groups_gen;
		rc = process_block_buses(c, rows, reuse ? nullptr : slots, n, F, d_out, n_buses, d_pk, GAS_MEM_DEVICE);
		c->streams.bus_staged = rc == GAS_OK && n > 0 && c->cached_n != n; // ran staged: nothing cached to compare with next time
	} else {
		rc = process_block(c, rows, same_list ? nullptr : slots, n, F, d_out, d_pk, GAS_MEM_DEVICE);
	}
	c->streams.groups_gen = rc == GAS_OK ? c->groups_gen : UINT64_MAX;
	GAS_TRY(rc);
	if (mem == GAS_MEM_DEVICE) {
		return GAS_OK;
	}
	if (!buses) {
		GAS_TRY(join_outputs(c));
	}
	GAS_HIP(c, copy_back(c, out, d_out, out_bytes, peaks, n));
	return GAS_OK;
}

// Both stream entries.  !buses: gas_process_block_streams (one mix, out [C][frames], n_buses unused); buses:
// gas_process_block_streams_buses (out [n_buses][C][frames]).
int process_block_streams(gas_ctx *c, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, uint32_t n_buses, bool buses, float *peaks, uint8_t *has_frames, int mem) {
	if (!c || !out || (n > 0 && !slots) || n > c->cfg.max_sources || (mem != GAS_MEM_HOST && mem != GAS_MEM_DEVICE)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	const size_t bus_bytes = (size_t)c->cfg.channel_count * c->cfg.frames * sizeof(gas_audio_frame);
	if (buses && (n_buses < 1 || n_buses > GAS_MAX_BUSES)) { // zeroes as much of `out` as a legal call could name
		return fail_out(GAS_ERR_INVALID_ARGUMENT, mem, out, (n_buses < GAS_MAX_BUSES ? n_buses : GAS_MAX_BUSES) * bus_bytes);
	}
	GAS_TRY(flush_deferred(c)); // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
	const size_t out_bytes = (buses ? n_buses : 1u) * bus_bytes;
	return fail_out(stream_body(c, slots, n, frames, out, out_bytes, n_buses, buses, peaks, has_frames, mem), mem, out, out_bytes);
}

} // namespace

extern "C" {

int gas_process_block(gas_ctx *c, const gas_audio_frame *src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, float *peaks, int mem) {
	if (!c || !out || (mem != GAS_MEM_HOST && mem != GAS_MEM_DEVICE) || (n > 0 && !src) || n > c->cfg.max_sources) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	return fail_out(process_block(c, RowSource{ src }, slots, n, frames, out, peaks, mem), mem, out, (size_t)c->cfg.channel_count * c->cfg.frames * sizeof(gas_audio_frame));
}

int gas_bus_routes_publish(gas_ctx *c, const uint32_t *slots, const gas_bus_route *routes, uint32_t n) {
	if (!c || (n > 0 && (!slots || !routes))) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	for (uint32_t i = 0; i < n; i++) {
		if (slots[i] >= c->cfg.max_sources || !c->slots[slots[i]].used) {
			return GAS_ERR_BAD_SLOT;
		}
	}
	std::lock_guard<std::mutex> lk(c->params_mu);
	for (uint32_t i = 0; i < n; i++) {
		c->h_routes[slots[i]] = routes[i];
	}
	c->routes_dirty = true;
	return GAS_OK;
}

int gas_process_block_buses(gas_ctx *c, const gas_audio_frame *src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, uint32_t n_buses, float *peaks, int mem) {
	if (!c || !out || (mem != GAS_MEM_HOST && mem != GAS_MEM_DEVICE) || (n > 0 && !src) || n > c->cfg.max_sources || n_buses < 1 || n_buses > GAS_MAX_BUSES) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	return process_block_buses(c, RowSource{ src }, slots, n, frames, out, n_buses, peaks, mem);
}

int gas_process_block_streams(gas_ctx *c, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, float *peaks, uint8_t *has_frames, int mem) {
	return process_block_streams(c, slots, n, frames, out, 0, false, peaks, has_frames, mem);
}

int gas_process_block_streams_buses(gas_ctx *c, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, uint32_t n_buses, float *peaks, uint8_t *has_frames, int mem) {
	return process_block_streams(c, slots, n, frames, out, n_buses, true, peaks, has_frames, mem);
}

int gas_stream_last_fused(gas_ctx *c) {
	return c ? (c->streams.last_fused ? 1 : 0) : GAS_ERR_INVALID_ARGUMENT;
}

int gas_process_frames_1(gas_ctx *c, uint32_t slot, gas_audio_frame *out, const gas_audio_frame *src, int frame_count) {
	return process_one(c, slot, 0, false, out, src, frame_count);
}

int gas_mix_channel_1(gas_ctx *c, uint32_t slot, int channel, gas_audio_frame *out, const gas_audio_frame *src, int frame_count) {
	return process_one(c, slot, channel, true, out, src, frame_count);
}

} // extern "C"
