// gas_ctx.hip -- the C ABI of include/gas_amd.h: context, device-resident playback-data slots,
// parameter publication, and the per-callback launch sequence that stands in for
// AudioSpatializerInstance::_mix_from_playback_list (audio_spatializer.cpp:326-471).
//
// There is NO CPU fallback: every entry needs a HIP device and fails with GAS_ERR_NO_DEVICE /
// GAS_ERR_DEVICE otherwise.
#include <algorithm>
#include <array>
#include <cmath>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <new>

#include "gas_fx_dyn_check.h"
#include "gas_fx_eq_check.h"
#include "gas_fx_filter_check.h"
#include "gas_fx_line_check.h"
#include "gas_fx_mod_check.h"
#include "gas_fx_stereo_check.h"
#include "gas_internal.h"
#include "gas_owned.h"
#include "gas_qoa.h"

namespace {

// Launch groups: sources of one callback that run the same kernel instantiation.
enum gas_group_type {
	G_3D_MIX = 0, // must stay first: only these write channel pairs > 0
	G_3D_PROCESS,
	G_FX_COPY,
	G_FX_SHELF,
	G_FX_ER,
	G_FX_HRTF, // frequency-domain accumulation, no per-source peak
	G_FX_HRTF_PK, // per-source inverse FFTs: exact peaks (draining playbacks / peaks-for-all contexts); launched with G_FX_HRTF
	G_FX_ER_HRTF,
	G_FX_ER_HRTF_PK, // launched with G_FX_ER_HRTF
	G_FX_GENERIC, // any other chain of the implemented effects: staged through ping-pong row buffers (audio_spatializer_effect.cpp:52-76)
	G_COUNT
};

const char *const k_group_kernel[G_COUNT] = {
	"k_biquad_mix<MIX_CHANNEL>", "k_biquad_mix<PROCESS_FRAMES>", "k_biquad_mix<COPY>", "k_biquad_mix<FX_HIGHSHELF>",
	"k_er_only", "k_hrtf_ols", "k_hrtf_ols", "k_hrtf_ols<ER>", "k_hrtf_ols<ER>", "staged effect chain"
};

struct SlotInfo {
	uint8_t used = 0;
	uint8_t kind = 0;
	uint8_t group = 0;
	uint8_t has_params = 0;
	uint8_t pending_free = 0;
	uint8_t dirty_state = 0; // state must be zeroed before reuse
	uint32_t chain_sig = 0; // G_FX_GENERIC: effect kinds, 8 bits each, first effect in the low byte
	uint8_t draining = 0; // stream ended: the host's silence gate needs this source's peak (audio_spatializer.cpp:464)
};

struct Group {
	uint32_t offset = 0, count = 0;
	bool contiguous = false; // the group's slots are slot_base, slot_base + 1, ... in order
	uint32_t slot_base = 0;
};

// One run of G_FX_GENERIC entries that share a chain.
struct ChainRange {
	uint32_t sig = 0;
	uint32_t offset = 0, count = 0; // relative to the group's offset
	bool peak_all = true, peak_any = true; // which of its sources report their exact peak (GAS_FLAG_PEAKS_DRAINING_ONLY; read by a last stage that is k_hrtf_uni)
};

// Which slots the current list has named so far, without a pass over every slot between two lists.
struct SlotStamp {
	std::vector<uint32_t> at; // [max_sources]: the list that named the slot last
	uint32_t gen = 0;
	void next() { // a new list begins
		if (++gen == 0) {
			std::fill(at.begin(), at.end(), 0u);
			gen = 1;
		}
	}
	bool has(uint32_t slot) const {
		return at[slot] == gen;
	}
	bool seen(uint32_t slot) { // true: named before in this list; marks it otherwise
		if (has(slot)) {
			return true;
		}
		at[slot] = gen;
		return false;
	}
};

constexpr uint32_t PROFILE_EVENTS = 4096;

// The effect families, in the order their uploads are flushed; k_fx_families describes them.  The
// first two have no pool: gas_fx_settings (GAS_FX_LOWPASS .. GAS_FX_AMPLIFY) and gas_fx_dyn_settings.
enum { FX_BASIC = 0, FX_DYN, FX_LINES, FX_EQ, FX_FILTER, FX_MOD, FX_STEREO, FX_FAMILIES };

// Host side of one family: pool sizes and free entries (alloc_mu), each slot's entries by chain position (written
// under alloc_mu and params_mu), the settings mirror and what the next flush uploads (params_mu):
// [m settings][m {slot, entry[4]}][z {pool, entry} zero records] through one pinned staging buffer.
struct FxFamily {
	uint32_t cap[2] = { 0, 0 };
	std::vector<uint32_t> free[2];
	std::vector<std::array<int32_t, GAS_MAX_EFFECTS>> h_of;
	std::vector<unsigned char> h_settings; // [max_sources] settings PODs, latest published value
	std::vector<uint8_t> dirty_flag;
	std::vector<uint32_t> dirty_list;
	std::vector<uint32_t> zero_list; // {pool, entry} zero records, each entry at most once (zero_pending)
	std::vector<uint8_t> zero_pending[2]; // [pool][entry]: queued in zero_list
	unsigned char *h_upload = nullptr, *d_upload = nullptr;
};

// gas_owned.h's way to the runtime: the only place that allocates or frees device memory, pinned memory or events.
struct HipMem {
	using status = hipError_t;
	using event = hipEvent_t;
	static constexpr status misuse = hipErrorInvalidValue;
	static status device_alloc(void **p, size_t bytes) {
		return hipMalloc(p, bytes);
	}
	static status device_free(void *p) {
		return hipFree(p);
	}
	static status pinned_alloc(void **p, size_t bytes) {
		return hipHostMalloc(p, bytes, hipHostMallocDefault);
	}
	static status pinned_free(void *p) {
		return hipHostFree(p);
	}
	static status event_create(event *e, unsigned flags) {
		return hipEventCreateWithFlags(e, flags);
	}
	static status event_destroy(event e) {
		return hipEventDestroy(e);
	}
};
using Mem = gas_owned<HipMem>;

} // namespace

struct gas_ctx {
	Mem mem; // owns every device buffer, pinned buffer and event below: they are allocated through it alone
	gas_config cfg{};
	hipStream_t stream = nullptr;
	bool own_stream = false;
	// GAS_FLAG_PIPELINED_MIX: the sum of callback t's partial mixes is carried out inside callback t+1's k_hrtf_ols
	// launch (or by gas_ctx_join_outputs / the next ordered call); two generations of partials alternate
	bool pipelined_mix = false;
	uint32_t pipe_tick = 0;
	struct PendingMix {
		int parity = 0; // plane of d_partials holding the callback's partial mixes
		uint32_t p_total = 0;
		gas_audio_frame *out = nullptr;
	};
	std::vector<PendingMix> pending; // the sums not launched yet, oldest first: one after a single launch, one per block after a batched one
	// GAS_FLAG_BATCHED_LAUNCH: plain-[HRTF] device-memory callbacks wait here until batch_depth of them run as ONE
	// k_hrtf_multi launch.  Anything that could change what the waiting callbacks must see runs them first.
	struct Deferred {
		const gas_audio_frame *src = nullptr;
		gas_audio_frame *out = nullptr;
		float *peaks = nullptr;
		const gas_params *fresh = nullptr;
	};
	std::vector<Deferred> deferred;
	uint32_t deferred_n = 0;
	uint64_t deferred_groups_gen = 0;
	uint32_t batch_depth = 2; // callbacks per launch (gas_ctx_set_batch_depth), <= GAS_HRTF_MULTI_MAX_BLOCKS
	int bus_form_cached = 0; // form of the last gas_process_block_buses whose list can be reused: 1 3D mix, 2 fused [HRTF], 0 none
	uint64_t bus_form_groups_gen = 0;
	uint32_t partial_planes = 1; // planes of d_partials (1 ordered, 2 pipelined, 2 x max batch depth batched)
	bool prof_multi = false; // the timed launch was k_hrtf_multi
	uint32_t hist_len = 0;
	gas_dev_state st{};
	gas_hrtf_table tab{};
	float2 *d_tw = nullptr;

	std::vector<SlotInfo> slots;
	std::vector<uint32_t> free_list;
	std::vector<uint32_t> pending_free; // audio thread: frees taking effect at the next block boundary
	std::mutex alloc_mu; // gas_source_alloc / gas_source_free may come from any thread: guards free_list and free_inbox
	std::vector<uint32_t> free_inbox; // frees requested since the audio thread last looked (adopt_frees)
	SlotStamp stamp; // duplicate detection per block
	SlotStamp calc_stamp; // the same for gas_calc_spatialization's slot list (physics thread, under calc_mu)

	std::mutex params_mu;
	gas_params *h_params = nullptr; // pinned [max_sources], latest published value
	std::vector<uint8_t> dirty_flag;
	std::vector<uint32_t> dirty_list;
	gas_params *h_upload = nullptr; // pinned
	uint32_t *h_upload_slots = nullptr; // pinned
	gas_params *d_upload = nullptr;
	uint32_t *d_upload_slots = nullptr;
	// gas_hrtf_blend rows (GAS_FLAG_HRTF_INTERPOLATE): host mirror, latest wins, uploaded with the parameters
	// (params_mu); empty without the flag
	std::vector<gas_hrtf_blend> h_blend;
	std::vector<uint8_t> blend_dirty_flag;
	std::vector<uint32_t> blend_dirty_list;
	gas_hrtf_blend *h_blend_upload = nullptr; // pinned, [max_sources], allocated by the first flush that needs it
	// the effect families, and what the reservations (gas_ctx_reserve_fx_*) derive from the mix rate
	FxFamily fx[FX_FAMILIES];
	gas_line_geo line_geo{};
	gas_eq_coefs eq_coefs[3] = {}; // EQ6, EQ10, EQ21 at the mix rate (make_eq_coefs)

	// plain [HRTF] group of the cached list (k_hrtf_uni): which entries need their exact peak
	uint32_t *h_peak_bits = nullptr, *d_peak_bits = nullptr; // two halves of (max_sources + 31) / 32 words: bit k = entry k of the plain-[HRTF] group / of the staged group
	bool uni_peak_all = false, uni_peak_any = false;
	uint32_t *h_idx = nullptr; // pinned [2 * max_sources]: slots then rows, sorted by group
	uint32_t *d_slots = nullptr, *d_rows = nullptr; // sorted by launch group
	uint32_t *d_slots_rows = nullptr; // the caller's list in row order (device-side parameter publication)
	uint32_t cached_n = UINT32_MAX;
	uint64_t groups_gen = 0; // bumped whenever build_groups re-sorts a slot list
	std::atomic<uint64_t> params_gen{ 1 }; // bumped by every call that can change a source's HRIR direction
	uint32_t *d_order = nullptr; // [max_sources] direction order of the frequency-domain HRTF groups (k_dir_order)
	uint64_t order_groups_gen = UINT64_MAX, order_params_gen = 0; // what d_order was built from
	bool order_ok[G_COUNT] = {}; // d_order holds this group's order
	uint32_t xcd_order_auto_min = GAS_XCD_ORDER_AUTO_MIN; // GAS_XCD_ORDER_AUTO_MIN in the environment overrides (experiments)
	bool last_uni_ordered = false; // the last k_hrtf_uni launch ran in k_xcd_order's order
	uint64_t stream_groups_gen = UINT64_MAX; // groups_gen the stream path's cached list corresponds to
	bool cached_identity_rows = true;
	Group groups[G_COUNT];
	std::vector<ChainRange> chain_ranges; // sub-runs of groups[G_FX_GENERIC], cached with the groups
	gas_audio_frame *d_chain[2] = { nullptr, nullptr }; // ping-pong rows of the staged chains
	size_t d_chain_frames = 0;

	gas_audio_frame *d_src = nullptr; // staging for GAS_MEM_HOST, lazily sized
	size_t d_src_frames = 0;
	// gas_sidechain_set(GAS_MEM_HOST): pinned staging per key, and the event behind each key's last copy out of it
	gas_audio_frame *h_sidechain = nullptr; // [GAS_MAX_SIDECHAINS][frames]
	hipEvent_t sidechain_ev[GAS_MAX_SIDECHAINS] = {};
	gas_audio_frame *d_out = nullptr; // [C][F]
	float *d_peaks = nullptr; // [max_sources][2]
	float *d_partials = nullptr;
	uint32_t partial_rows = 0; // rows per channel pair

	// one-source compatibility path
	uint32_t *d_one_slot = nullptr;

	// device-resident streams and playback cursors
	struct StreamInfo {
		void *d_pcm = nullptr;
		uint64_t frames = 0;
		uint32_t format = 0, channels = 0;
		bool resampled = false; // its playbacks are [ENGINE] AudioStreamPlaybackResampled (gas_stream_set_resampled)
		uint32_t loop_mode = 0; // NEW gas_stream_set_loop: its playbacks repeat [loop_begin, loop_end)
		uint64_t loop_begin = 0, loop_end = 0;
	};
	std::vector<StreamInfo> streams;
	gas_cursor *d_cursors = nullptr; // [max_sources]
	std::vector<gas_cursor> h_cursors; // host mirror of the cursor arithmetic (deterministic, no read-back)
	float *d_fade_env = nullptr; // [64]
	uint32_t *d_stream_slots = nullptr; // callback slot list in row order
	uint32_t *d_stream_inc = nullptr, *h_stream_inc = nullptr; // [max_sources] 16.16 step per row (resampled playbacks)
	bool stream_any_resampled = false;
	std::vector<uint32_t> stream_slots_host; // what d_stream_slots / the cached launch groups currently hold
	// parameter rows published from device memory for the cached slot list (row order), not yet in the table
	const gas_params *pending_params = nullptr;
	uint32_t pending_n = 0;
	struct StreamRow { // compact mirror of the cached list's cursors: the per-callback host loop touches only this
		uint64_t remaining = 0;
		uint32_t has_frames = 0, draining_marked = 0;
		uint32_t resampled = 0, inc = 65536; // resampled playbacks: 16.16 step of this callback (from the host-published pitch_scale)
		uint64_t fp_pos = 0, end_fp = 0; // ... and the engine's mix_offset / the stream's end, 16.16
		uint32_t looped = 0; // gas_stream_set_loop: never ends; a plain playback counts `pos` up instead of `remaining` down
		uint64_t pos = 0;
	};
	std::vector<StreamRow> stream_rows;
	bool stream_all_hrtf = false;
	bool stream_last_fused = false; // the last stream callback that got as far as its launches sampled inside the HRTF kernel (gas_stream_last_fused)
	bool stream_last_buses = false; // the cached stream list was validated by gas_process_block_streams_buses (its checks differ from the mix entry's)
	bool stream_bus_staged = false; // ... and ran the staged bus form, which regroups on every call (cached_n never names it)
	bool stream_rows_first = getenv("GAS_STREAM_ROWS_FIRST") != nullptr && atoi(getenv("GAS_STREAM_ROWS_FIRST")) != 0; // development aid: plain [HRTF] stream lists sample rows first too (tools/time_stream_loops.py compares the routes)
	bool stream_any_looped = false;
	bool stream_any_adpcm = false; // the list holds a GAS_PCM_IMA_ADPCM playback: rows first, k_sample_adpcm behind k_sample_sources
	bool adpcm_span = getenv("GAS_ADPCM_SPAN") == nullptr || atoi(getenv("GAS_ADPCM_SPAN")) != 0; // development aid: 0 = every load decodes from its checkpoint (k_sample_adpcm.hip; tools/time_stream_adpcm.py and the tests compare the paths)
	bool stream_any_qoa = false; // the list holds a GAS_PCM_QOA playback: rows first, k_sample_qoa behind k_sample_sources
	bool qoa_span = getenv("GAS_QOA_SPAN") == nullptr || atoi(getenv("GAS_QOA_SPAN")) != 0; // development aid: 0 = every load decodes from its record (k_sample_qoa.hip; tools/time_stream_qoa.py and the tests compare the paths)
	bool stream_params_touched = false; // a parameter publish may have changed pitch_scale: re-validate
	// gas_source_feed_rows: window rows of playbacks that are not bound to a stream, pending for the next stream callback.
	// d_feed is the feed table the kernels read (gas_internal.h, GAS_FEED_*): [max_sources] words in the callback's row
	// order, then two halves of max_sources rows: the rows of every call since the last callback, appended as they came
	// (feed_place).
	uint8_t *d_feed = nullptr;
	size_t feed_used = 0; // end of the rows taken, as an offset into d_feed (0: emptied)
	uint32_t feed_side = 0; // the half of the table that rows are appended in
	std::vector<uint32_t> feed_moved; // feed_place: (slot, new word) of the rows it moved to the other half
	uint8_t *h_feed = nullptr; // pinned staging of one GAS_MEM_HOST call
	size_t h_feed_cap = 0;
	hipEvent_t feed_ev = nullptr; // the last upload out of h_feed
	std::vector<uint32_t> feed_word; // [max_sources] by slot: GAS_FEED_NONE, or where and in which format its pending row lies
	std::vector<uint32_t> feed_slots; // the slots with a pending row
	std::vector<uint32_t> feed_entry, feed_entry_dev; // per list entry: this callback's words, and the words the table's header holds (empty: none written)
	uint32_t *h_feed_entry = nullptr; // [max_sources] pinned: what the header upload reads
	hipEvent_t feed_entry_ev = nullptr; // ... and the last upload out of it

	// gas_calc_spatialization staging (physics thread)
	std::mutex calc_mu;
	gas_spatializer3d_config *d_calc_cfgs = nullptr;
	gas_listener *d_calc_listeners = nullptr;
	uint32_t *d_calc_slots = nullptr, *d_calc_cfgidx = nullptr;
	gas_source_pose *d_calc_poses = nullptr;
	gas_params *d_calc_out = nullptr;
	gas_area_send *d_calc_areas = nullptr; // gas_calc_spatialization_areas staging (host-memory calls)
	float *d_calc_lap = nullptr;
	gas_audio_frame *d_calc_reverb = nullptr;
	gas_room *d_calc_rooms = nullptr; // gas_calc_early_reflections: its rooms (everything else it stages lies in the buffers above)

	// several output buses: slot-indexed routes, host mirror + device table, own partial planes
	std::vector<gas_bus_route> h_routes; // guarded by params_mu
	bool routes_dirty = false;
	gas_bus_route *h_routes_pinned = nullptr, *d_routes = nullptr;
	float *d_bus_partials = nullptr;
	size_t bus_partial_floats = 0;
	gas_audio_frame *d_bus_out = nullptr; // [GAS_MAX_BUSES][C][F] staging for host-memory calls

	// bus convolvers (gas_conv_*, NEW): pools, tables and staging are gas_ctx_reserve_conv's, an IR's spectra
	// gas_conv_ir_load's; the instance calls and gas_conv_process allocate nothing.  Audio-thread state, no lock: the
	// reservation and the IR calls never run concurrently with a callback.
	struct ConvIr {
		float2 *H = nullptr; // [channels][k_ir][GAS_CONV_BINS]; null: a free id
		uint32_t channels = 0, taps = 0, k_ir = 0;
		uint32_t users = 0; // references from instances: a state, a fade's target and a pending target each count
	};
	struct ConvTarget {
		uint32_t ir = 0;
		float dry = 0.0f, wet = 1.0f;
	};
	struct ConvInst {
		bool used = false;
		uint32_t ir = 0;
		uint32_t pos = 0; // ring position of the newest spectrum
		float dry = 0.0f, wet = 1.0f;
		// gas_conv_fade_to: (ir, dry, wet) above is state A; fade_n > 0: fading to `to`, fade_pos of fade_n calls made
		uint32_t fade_n = 0, fade_pos = 0;
		ConvTarget to;
		uint32_t pending_n = 0; // > 0: `pending` starts, over pending_n calls, when the fade in progress has ended
		ConvTarget pending;
	};
	uint32_t conv_count = 0, conv_max_taps = 0; // the reservation; 0: none
	gas_conv_pool conv_pool{};
	float2 *conv_w1024 = nullptr;
	std::vector<ConvInst> conv;
	std::vector<uint32_t> conv_free; // pop_back hands out 0, 1, 2, ...
	std::vector<ConvIr> conv_irs;
	gas_audio_frame *conv_h_in = nullptr, *conv_h_out = nullptr; // pinned [GAS_MAX_CONVOLVERS][frames], host-memory calls
	gas_audio_frame *conv_d_in = nullptr, *conv_d_out = nullptr;

	// gas_bandwidth_probe: read arena (larger than the Infinity Cache, swept in rotation) and write target
	void *d_probe_rd = nullptr, *d_probe_wr = nullptr;
	size_t probe_rd_bytes = 0, probe_wr_bytes = 0;
	float *d_probe_sink = nullptr;

	bool profiling = false;
	std::vector<hipEvent_t> ev;
	uint32_t ev_used = 0;
	uint64_t prof_launches = 0;
	double prof_ms = 0.0;
	uint64_t prof_bytes = 0, prof_bytes_formula = 0;
	uint32_t prof_k = 1;
	int prof_group = -1;
	bool prof_uni = false; // the timed launch was k_hrtf_uni
	bool uni_flt_enabled = getenv("GAS_UNI_FLT") == nullptr || atoi(getenv("GAS_UNI_FLT")) != 0; // [filter, HRTF] through k_hrtf_uni<FLT> (0: the filter stage and the HRTF stage as two launches, for comparison)
	// [ER, HRTF] through k_hrtf_uni<ER>.  GAS_UNI_ER = 1 (default): when at most a quarter of the callback's playbacks want
	// their exact peak.  In throughput mode it is the faster form (the launch carries the previous callback's sum, which
	// k_hrtf_ols<ER> has no registers to park: 20.4 vs 22.4 us for cfg5), an ordered callback is a tie (22.7 / 22.4 us) --
	// the choice does not look at the mode, so the two modes stay bit-identical -- and with every peak exact the split
	// kernel's exact-peak workgroups win (23.6 vs 25.8 us).  0: never.  2: always (tests, A/B).  Staged chains that END in
	// [ER, HRTF] take it whenever it is not 0 (one launch less, no rows in between).
	int uni_er_mode = getenv("GAS_UNI_ER") ? atoi(getenv("GAS_UNI_ER")) : 1;
	bool uni_er_enabled = uni_er_mode != 0;
	bool prof_pipe = false; // the timed launch was k_biquad_pipe
	double ev_overhead_ms = 0.0; // marker/dispatch overhead of an event pair around one launch (calibrated)
	uint32_t prof_every = 1, prof_tick = 0; // bracket every Nth callback's dominant launch

	std::string last_err;
};

namespace {

#define GAS_HIP(ctx, call)                                                                    \
	do {                                                                                      \
		hipError_t _e = (call);                                                               \
		if (_e != hipSuccess) {                                                               \
			(ctx)->last_err = std::string(#call) + ": " + hipGetErrorString(_e);              \
			return GAS_ERR_DEVICE;                                                            \
		}                                                                                     \
	} while (0)

// Returns the status of `expr` to the caller unless it is GAS_OK.
#define GAS_TRY(expr)               \
	do {                            \
		const int _rc = (expr);     \
		if (_rc != GAS_OK) {        \
			return _rc;             \
		}                           \
	} while (0)

// The slot names a playback of this context.
inline bool live(const gas_ctx *c, uint32_t slot) {
	return slot < c->cfg.max_sources && c->slots[slot].used;
}

// A lazily allocated buffer: each pointer is guarded by its own null test.
template <class T>
hipError_t alloc_once(gas_ctx *c, T *&p, size_t count, Mem::Kind kind = Mem::DEVICE) {
	return p ? hipSuccess : c->mem.alloc(p, count, kind);
}

// `count` zeroed elements: the fill runs on the context's stream.
template <class T>
hipError_t device_zeroed(gas_ctx *c, T *&p, size_t count) {
	const hipError_t e = c->mem.alloc(p, count);
	return e != hipSuccess ? e : hipMemsetAsync(p, 0, count * sizeof(T), c->stream);
}

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
		if (a.use_order && ((c->cfg.flags & GAS_FLAG_XCD_ORDER) != 0 || g_fd.n >= c->xcd_order_auto_min) && uni_wgs % 8 == 0 && c->tab.dirs >= 8) {
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
		if (last_is_uni && c->uni_flt_enabled && (r.sig >> 8) == GAS_FX_HRTF && (k0 == GAS_FX_HIGHSHELF || (k0 >= GAS_FX_LOWPASS && k0 <= GAS_FX_LOWSHELF)) && gas_shelf_scan_applies(k0 == GAS_FX_HIGHSHELF ? GAS_MODE_FX_HIGHSHELF : GAS_MODE_FX_FILTER, r.count, F)) {
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
				GAS_HIP(c, gas_launch_biquad_mix(c->stream, GAS_MODE_FX_HIGHSHELF, in, c->st, F, (uint32_t)j, 1, c->cfg.mix_rate, run.parts, 0, c->partial_rows, reinterpret_cast<float *>(outb)));
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
	const bool uni_er_pays = c->uni_er_mode == 2 || groups[G_FX_ER_HRTF_PK].count * 4 <= groups[G_FX_ER_HRTF].count + groups[G_FX_ER_HRTF_PK].count;
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
		const bool timed = c->profiling && gt == dom && c->ev_used + 2 <= c->ev.size() && (c->prof_tick++ % c->prof_every) == 0;
		if (timed) {
			GAS_HIP(c, hipEventRecord(c->ev[c->ev_used], c->stream));
		}
		uint64_t carried = 0; // bytes of the previous callback's partial mixes summed inside this launch (GAS_FLAG_PIPELINED_MIX)
		switch (gt) {
			case G_3D_MIX:
			case G_3D_PROCESS: {
				int mode = gt == G_3D_MIX ? GAS_MODE_MIX_CHANNEL : GAS_MODE_PROCESS_FRAMES;
				if (a.force_mode >= 0) {
					mode = a.force_mode;
				}
				const uint32_t cb = mode == GAS_MODE_MIX_CHANNEL ? a.channel_begin : 0;
				const uint32_t cc = mode == GAS_MODE_MIX_CHANNEL ? a.channel_count : 1;
				GAS_HIP(c, gas_launch_biquad_mix(c->stream, mode, ga, c->st, F, cb, cc, c->cfg.mix_rate, parts, run.p_off, c->partial_rows));
			} break;
			case G_FX_COPY:
				GAS_HIP(c, gas_launch_biquad_mix(c->stream, GAS_MODE_COPY, ga, c->st, F, 0, 1, c->cfg.mix_rate, parts, run.p_off, c->partial_rows));
				break;
			case G_FX_SHELF:
				GAS_HIP(c, gas_launch_biquad_mix(c->stream, GAS_MODE_FX_HIGHSHELF, ga, c->st, F, 0, 1, c->cfg.mix_rate, parts, run.p_off, c->partial_rows));
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
			GAS_HIP(c, hipEventRecord(c->ev[c->ev_used + 1], c->stream));
			c->ev_used += 2;
			c->prof_bytes = group_bytes(c, gt, gr.count) + carried;
			c->prof_k = 1;
			if ((gt == G_FX_HRTF || gt == G_FX_ER_HRTF) && groups[gt + 1].count > 0) {
				// the exact-peak sources ride in the same launch: add their per-source bytes (table/mix terms counted once)
				c->prof_bytes += group_bytes(c, gt + 1, groups[gt + 1].count) - group_bytes(c, gt + 1, 0);
			}
			c->prof_group = gt;
			c->prof_uni = (gt == G_FX_HRTF && run.uni_hrtf && groups[G_FX_HRTF_PK].count == 0) || ((gt == G_FX_ER_HRTF || gt == G_FX_ER_HRTF_PK) && run.uni_er);
			c->prof_multi = false;
			c->prof_pipe = (gt == G_3D_MIX || gt == G_3D_PROCESS || gt == G_FX_SHELF) && gas_biquad_uses_pipe(gt == G_FX_SHELF ? GAS_MODE_FX_HIGHSHELF : (a.force_mode >= 0 ? a.force_mode : (gt == G_3D_MIX ? GAS_MODE_MIX_CHANNEL : GAS_MODE_PROCESS_FRAMES)), gr.count, gt == G_3D_MIX ? a.channel_count : 1, F, false);
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
	const bool timed = c->profiling && c->ev_used + 2 <= c->ev.size() && (c->prof_tick++ % c->prof_every) == 0;
	if (timed) {
		GAS_HIP(c, hipEventRecord(c->ev[c->ev_used], c->stream));
	}
	GAS_HIP(c, gas_launch_hrtf_multi(c->stream, ga, mb, plain_peak_bits(c), c->uni_peak_all, c->st, c->tab, c->d_tw, F, c->hist_len, c->d_partials));
	if (timed) {
		GAS_HIP(c, hipEventRecord(c->ev[c->ev_used + 1], c->stream));
		c->ev_used += 2;
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
			c->prof_bytes = (uint64_t)K * n * (F * 8 + 8) + fresh_blocks * n * 8 + (uint64_t)n * 8 + (hist_lds ? 1ull : (uint64_t)K) * n * hist_rw + (uint64_t)c->tab.dirs * 2 * GAS_HRTF_TAPS * 4 + (uint64_t)K * c->cfg.channel_count * F * 8 + carried;
		}
		c->prof_bytes_formula = (uint64_t)K * group_bytes(c, G_FX_HRTF, n) + carried;
		c->prof_k = K;
		c->prof_group = G_FX_HRTF;
		c->prof_uni = false;
		c->prof_pipe = false;
		c->prof_multi = true;
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
				return gas_launch_biquad_mix(c->stream, kind == GAS_FX_AMPLIFY ? GAS_MODE_FX_AMPLIFY : GAS_MODE_FX_FILTER, in, c->st, c->cfg.frames, j, 1, c->cfg.mix_rate, c->d_partials, 0, c->partial_rows, reinterpret_cast<float *>(out), gas_bus_args(), kind);
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

int flush_params(gas_ctx *c) {
	int rc = flush_param_rows(c);
	rc = rc != GAS_OK ? rc : fx_flush(c, FX_BASIC); // (the blend rows keep their place between the first two families)
	rc = rc != GAS_OK ? rc : flush_hrtf_blend(c);
	for (int f = FX_BASIC + 1; f < FX_FAMILIES && rc == GAS_OK; f++) {
		rc = fx_flush(c, f);
	}
	return rc;
}

void stream_rows_sync_back(gas_ctx *c);

// gas_source_feed_rows: forget the slot's pending row.  Its bytes of the feed table stay taken until the next stream
// callback empties the table (or feed_place moves on to the table's other half).
void feed_drop(gas_ctx *c, uint32_t slot) {
	if (c->feed_word[slot] == GAS_FEED_NONE) {
		return;
	}
	c->feed_word[slot] = GAS_FEED_NONE;
	auto it = std::find(c->feed_slots.begin(), c->feed_slots.end(), slot);
	*it = c->feed_slots.back();
	c->feed_slots.pop_back();
}

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
		had_stream = had_stream || c->h_cursors[s].pcm != nullptr;
	}
	if (had_stream) {
		stream_rows_sync_back(c); // the compact mirror may still name these slots: fold it back before they are cleared
		c->stream_groups_gen = UINT64_MAX;
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
		if (c->h_cursors[s].pcm) {
			// a freed playback lets go of its stream (gas_stream_destroy must not see it as bound for ever, and a
			// re-allocated slot must not inherit the cursor): host mirror and device cursor both
			c->h_cursors[s] = gas_cursor{};
			GAS_HIP(c, hipMemsetAsync(c->d_cursors + s, 0, sizeof(gas_cursor), c->stream));
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
	if (er_fade_on(c)) { // the fused [ER, HRTF] kernels have no fading form: the tail of a staged chain stays two launches, whatever GAS_UNI_ER says
		c->uni_er_enabled = false;
	}
	if (const char *v = std::getenv("GAS_XCD_ORDER_AUTO_MIN")) {
		c->xcd_order_auto_min = (uint32_t)std::strtoul(v, nullptr, 10);
	}
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
		GAS_HIP(c, device_zeroed(c, c->d_cursors, N));
		GAS_HIP(c, c->mem.alloc(c->d_stream_slots, N));
		GAS_HIP(c, c->mem.alloc(c->d_stream_inc, N));
		GAS_HIP(c, c->mem.alloc(c->h_stream_inc, N, Mem::PINNED));
		c->feed_word.assign(N, GAS_FEED_NONE);
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
		GAS_HIP(c, c->mem.alloc(c->d_calc_cfgs, GAS_MAX_SPATIALIZER_CONFIGS));
		GAS_HIP(c, c->mem.alloc(c->d_calc_listeners, GAS_MAX_LISTENERS));
		GAS_HIP(c, c->mem.alloc(c->d_calc_slots, N));
		GAS_HIP(c, c->mem.alloc(c->d_calc_cfgidx, N));
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
	c->h_cursors.assign(N, gas_cursor{});
	c->stamp.at.assign(N, 0);
	c->calc_stamp.at.assign(N, 0);
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
	c->stream_params_touched = true;
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
		c->stream_params_touched = true;
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

int gas_calc_spatialization(gas_ctx *c, const gas_spatializer3d_config *cfgs, uint32_t n_cfgs, const uint32_t *cfg_index, const gas_source_pose *poses, const gas_listener *listeners, uint32_t n_listeners, const uint32_t *slots, uint32_t n, gas_params *out_params, int mem) {
	return gas_calc_spatialization_areas(c, cfgs, n_cfgs, cfg_index, poses, listeners, n_listeners, slots, n, nullptr, nullptr, out_params, nullptr, mem);
}

int gas_calc_spatialization_areas(gas_ctx *c, const gas_spatializer3d_config *cfgs, uint32_t n_cfgs, const uint32_t *cfg_index, const gas_source_pose *poses, const gas_listener *listeners, uint32_t n_listeners, const uint32_t *slots, uint32_t n, const gas_area_send *areas, const float *listener_area_pos, gas_params *out_params, gas_audio_frame *out_reverb, int mem) {
	if (!c || !cfgs || !poses || !slots || (n_listeners && !listeners) || (mem != GAS_MEM_HOST && mem != GAS_MEM_DEVICE)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (n_cfgs == 0 || n_cfgs > GAS_MAX_SPATIALIZER_CONFIGS || n_listeners > GAS_MAX_LISTENERS || n > c->cfg.max_sources) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	GAS_TRY(flush_deferred(c)); // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
	for (uint32_t i = 0; i < n_cfgs; i++) {
		if (cfgs[i].speaker_mode < 0 || cfgs[i].speaker_mode > 3 || !(cfgs[i].unit_size > 0.0f)) {
			return GAS_ERR_INVALID_ARGUMENT;
		}
	}
	for (uint32_t i = 0; i < n; i++) {
		if (!live(c, slots[i])) {
			return GAS_ERR_BAD_SLOT;
		}
		if (cfg_index && cfg_index[i] >= n_cfgs) {
			return GAS_ERR_INVALID_ARGUMENT;
		}
	}
	if (n == 0) {
		return GAS_OK;
	}
	std::lock_guard<std::mutex> lk(c->calc_mu);
	c->calc_stamp.next();
	for (uint32_t i = 0; i < n; i++) {
		if (c->calc_stamp.seen(slots[i])) {
			return GAS_ERR_INVALID_ARGUMENT; // one playback twice: two lanes would race on its table row and its latch
		}
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_TRY(flush_pending_params(c));
	{ // rows published from the host before this call reach the table first: the launch keeps their fields it does not
	  // write (early reflections, shelf, hrtf_* without a grid) and its own are not overwritten by them at the next callback
		int rcr = flush_param_rows(c);
		if (rcr != GAS_OK) {
			return rcr;
		}
	}
	{ // GAS_FLAG_HRTF_INTERPOLATE: blend rows published before this call reach the table first, so the launch's rows win
		int rcb = flush_hrtf_blend(c);
		if (rcb != GAS_OK) {
			return rcb;
		}
	}
	GAS_HIP(c, hipMemcpyAsync(c->d_calc_cfgs, cfgs, sizeof(gas_spatializer3d_config) * n_cfgs, hipMemcpyHostToDevice, c->stream));
	if (n_listeners) {
		GAS_HIP(c, hipMemcpyAsync(c->d_calc_listeners, listeners, sizeof(gas_listener) * n_listeners, hipMemcpyHostToDevice, c->stream));
	}
	GAS_HIP(c, hipMemcpyAsync(c->d_calc_slots, slots, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
	if (cfg_index) {
		GAS_HIP(c, hipMemcpyAsync(c->d_calc_cfgidx, cfg_index, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
	}
	const gas_source_pose *d_poses = poses;
	gas_params *d_out = out_params;
	if (mem == GAS_MEM_HOST) {
		GAS_HIP(c, alloc_once(c, c->d_calc_poses, c->cfg.max_sources));
		GAS_HIP(c, hipMemcpyAsync(c->d_calc_poses, poses, sizeof(gas_source_pose) * n, hipMemcpyHostToDevice, c->stream));
		d_poses = c->d_calc_poses;
		if (out_params) {
			GAS_HIP(c, alloc_once(c, c->d_calc_out, c->cfg.max_sources));
			d_out = c->d_calc_out;
		}
	}
	const gas_area_send *d_areas = areas;
	const float *d_lap = listener_area_pos;
	gas_audio_frame *d_reverb = out_reverb;
	if (mem == GAS_MEM_HOST && (areas || out_reverb)) { // staged like the poses; sized for the worst case once
		GAS_HIP(c, alloc_once(c, c->d_calc_areas, c->cfg.max_sources));
		GAS_HIP(c, alloc_once(c, c->d_calc_lap, (size_t)3 * GAS_MAX_LISTENERS * c->cfg.max_sources));
		GAS_HIP(c, alloc_once(c, c->d_calc_reverb, (size_t)4 * c->cfg.max_sources));
		if (areas) {
			GAS_HIP(c, hipMemcpyAsync(c->d_calc_areas, areas, sizeof(gas_area_send) * n, hipMemcpyHostToDevice, c->stream));
			d_areas = c->d_calc_areas;
		}
		if (listener_area_pos) {
			GAS_HIP(c, hipMemcpyAsync(c->d_calc_lap, listener_area_pos, sizeof(float) * 3 * n_listeners * n, hipMemcpyHostToDevice, c->stream));
			d_lap = c->d_calc_lap;
		}
		if (out_reverb) {
			d_reverb = c->d_calc_reverb;
		}
	}
	GAS_HIP(c, gas_launch_calc_spatialization(c->stream, c->d_calc_cfgs, cfg_index ? c->d_calc_cfgidx : nullptr, d_poses, c->d_calc_listeners, n_listeners, c->d_calc_slots, n, c->st.params, c->st.was_further, d_out, d_areas, d_lap, d_reverb, c->st.hrtf_blend));
	if (mem == GAS_MEM_HOST && out_params) {
		GAS_HIP(c, hipMemcpyAsync(out_params, c->d_calc_out, sizeof(gas_params) * n, hipMemcpyDeviceToHost, c->stream));
	}
	if (mem == GAS_MEM_HOST && out_reverb) {
		GAS_HIP(c, hipMemcpyAsync(out_reverb, c->d_calc_reverb, sizeof(gas_audio_frame) * 4 * n, hipMemcpyDeviceToHost, c->stream));
	}
	GAS_HIP(c, hipStreamSynchronize(c->stream)); // the host staging arrays are the caller's
	for (uint32_t i = 0; i < n; i++) {
		c->slots[slots[i]].has_params = 1;
	}
	return GAS_OK;
}

int gas_calc_early_reflections(gas_ctx *c, const gas_room *rooms, uint32_t n_rooms, const uint32_t *room_index, const gas_source_pose *poses, const gas_listener *listener, const uint32_t *slots, uint32_t n, gas_er_taps *out_taps, int mem) {
	if (!c || !rooms || !poses || !listener || (!slots && !out_taps) || (mem != GAS_MEM_HOST && mem != GAS_MEM_DEVICE)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (n_rooms == 0 || n_rooms > GAS_MAX_ROOMS || n > c->cfg.max_sources || c->cfg.er_ring_frames == 0) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	for (uint32_t r = 0; r < n_rooms; r++) {
		const gas_room &R = rooms[r];
		bool ok = R.speed_of_sound > 0.0f && std::isfinite(R.speed_of_sound) && R.level >= 0.0f && std::isfinite(R.level) && (R.max_order == 1 || R.max_order == 2);
		for (int a = 0; a < 3; a++) {
			ok = ok && R.half_extent[a] > 0.0f && std::isfinite(R.half_extent[a]);
		}
		for (int w = 0; w < 6; w++) {
			ok = ok && R.reflectance[w] >= 0.0f && R.reflectance[w] <= 1.0f;
		}
		if (!ok) {
			return GAS_ERR_INVALID_ARGUMENT;
		}
	}
	for (uint32_t i = 0; i < n; i++) {
		if (slots && !live(c, slots[i])) {
			return GAS_ERR_BAD_SLOT;
		}
		if (room_index && room_index[i] >= n_rooms && room_index[i] != GAS_ROOM_NONE) {
			return GAS_ERR_INVALID_ARGUMENT;
		}
	}
	if (n == 0) {
		return GAS_OK;
	}
	std::lock_guard<std::mutex> lk(c->calc_mu);
	if (slots) {
		c->calc_stamp.next();
		for (uint32_t i = 0; i < n; i++) {
			if (c->calc_stamp.seen(slots[i])) {
				return GAS_ERR_INVALID_ARGUMENT; // one playback twice: two lane groups would race on its row
			}
		}
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	if (slots) { // the launch writes table rows: whatever must still see or precede the old ones goes first.  Without
		// slots the launch reads and writes nothing of the context's but the staging buffers
		int rc = flush_deferred(c); // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch
		rc = rc != GAS_OK ? rc : flush_pending_params(c);
		rc = rc != GAS_OK ? rc : flush_param_rows(c); // host-published rows first: the launch's two fields land on top of them
		if (rc != GAS_OK) {
			return rc;
		}
	}
	GAS_HIP(c, alloc_once(c, c->d_calc_rooms, GAS_MAX_ROOMS));
	GAS_HIP(c, hipMemcpyAsync(c->d_calc_rooms, rooms, sizeof(gas_room) * n_rooms, hipMemcpyHostToDevice, c->stream));
	GAS_HIP(c, hipMemcpyAsync(c->d_calc_listeners, listener, sizeof(gas_listener), hipMemcpyHostToDevice, c->stream));
	if (slots) {
		GAS_HIP(c, hipMemcpyAsync(c->d_calc_slots, slots, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
	}
	if (room_index) { // config indices and room indices never travel in the same call
		GAS_HIP(c, hipMemcpyAsync(c->d_calc_cfgidx, room_index, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
	}
	const gas_source_pose *d_poses = poses;
	gas_er_taps *d_taps = out_taps;
	if (mem == GAS_MEM_HOST) {
		GAS_HIP(c, alloc_once(c, c->d_calc_poses, c->cfg.max_sources));
		GAS_HIP(c, hipMemcpyAsync(c->d_calc_poses, poses, sizeof(gas_source_pose) * n, hipMemcpyHostToDevice, c->stream));
		d_poses = c->d_calc_poses;
		if (out_taps) { // staged in the read-back buffer of gas_calc_spatialization's rows: a gas_er_taps is half a row
			static_assert(sizeof(gas_er_taps) <= sizeof(gas_params), "gas_er_taps are staged in d_calc_out");
			GAS_HIP(c, alloc_once(c, c->d_calc_out, c->cfg.max_sources));
			d_taps = reinterpret_cast<gas_er_taps *>(c->d_calc_out);
		}
	}
	GAS_HIP(c, gas_launch_calc_er(c->stream, c->d_calc_rooms, room_index ? c->d_calc_cfgidx : nullptr, d_poses, c->d_calc_listeners, c->d_calc_slots, n, c->cfg.er_ring_frames - c->cfg.frames, c->cfg.mix_rate, slots ? c->st.params : nullptr, d_taps));
	if (mem == GAS_MEM_HOST && out_taps) {
		GAS_HIP(c, hipMemcpyAsync(out_taps, d_taps, sizeof(gas_er_taps) * n, hipMemcpyDeviceToHost, c->stream));
	}
	GAS_HIP(c, hipStreamSynchronize(c->stream)); // the host staging arrays are the caller's
	return GAS_OK;
}

static inline void stream_rows_sync_back_fwd(gas_ctx *c) {
	stream_rows_sync_back(c);
}

int gas_stream_create(gas_ctx *c, const void *pcm, int format, uint32_t channels, uint64_t frames, uint32_t *out_stream) {
	if (!c || !pcm || !out_stream || (format != GAS_PCM_S16 && format != GAS_PCM_F32 && format != GAS_PCM_IMA_ADPCM && format != GAS_PCM_QOA) || (channels != 1 && channels != 2) || frames == 0) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (format == GAS_PCM_QOA && !gas_qoa_validate(static_cast<const uint8_t *>(pcm), gas_qoa_file_bytes(frames, channels), channels, frames)) {
		return GAS_ERR_INVALID_ARGUMENT; // the magic first: nothing else is read of data that are no QOA file
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	size_t bytes = (size_t)frames * channels * (format == GAS_PCM_S16 ? 2 : 4);
	std::vector<uint8_t> adpcm; // codes padded to whole chunks ++ checkpoint table (gas_internal.h)
	if (format == GAS_PCM_IMA_ADPCM) {
		bytes = (size_t)gas_adpcm_device_bytes(frames, channels);
		try {
			adpcm.assign(bytes, 0);
		} catch (const std::exception &) { // a length no host can stage
			return GAS_ERR_OUT_OF_MEMORY;
		}
		std::memcpy(adpcm.data(), pcm, (size_t)((frames + 1) / 2) * channels);
		gas_adpcm_ckpt *table = reinterpret_cast<gas_adpcm_ckpt *>(adpcm.data() + gas_adpcm_table_offset(frames, channels));
		for (uint32_t ch = 0; ch < channels; ch++) { // decode once, keeping the state in front of every chunk
			int32_t predictor = 0, step_index = 0;
			for (uint64_t i = 0; i < frames; i++) {
				if (i % GAS_ADPCM_CHUNK == 0) {
					table[(i / GAS_ADPCM_CHUNK) * channels + ch] = gas_adpcm_ckpt{ (int16_t)predictor, (uint8_t)step_index, 0 };
				}
				const uint32_t n = (adpcm[(i >> 1) * channels + ch] >> ((i & 1) * 4)) & 15u;
				gas_adpcm_step(predictor, step_index, n, gas_adpcm_step_size((uint32_t)step_index));
			}
		}
		pcm = adpcm.data();
	}
	std::vector<gas_qoa_record> qoa; // [chunk][channel] (gas_qoa.h)
	if (format == GAS_PCM_QOA) {
		bytes = (size_t)gas_qoa_device_bytes(frames, channels);
		try {
			qoa.assign(bytes / sizeof(gas_qoa_record), gas_qoa_record{});
		} catch (const std::exception &) {
			return GAS_ERR_OUT_OF_MEMORY;
		}
		gas_qoa_build_records(static_cast<const uint8_t *>(pcm), channels, frames, qoa.data()); // decodes once, keeping the state in front of every chunk
		pcm = qoa.data();
	}
	gas_ctx::StreamInfo si;
	GAS_HIP(c, c->mem.alloc(si.d_pcm, bytes));
	hipError_t e = hipMemcpy(si.d_pcm, pcm, bytes, hipMemcpyHostToDevice);
	if (e != hipSuccess) {
		c->mem.drop(si.d_pcm);
		c->last_err = hipGetErrorString(e);
		return GAS_ERR_DEVICE;
	}
	si.frames = frames;
	si.format = (uint32_t)format;
	si.channels = channels;
	for (size_t i = 0; i < c->streams.size(); i++) {
		if (!c->streams[i].d_pcm) {
			c->streams[i] = si;
			*out_stream = (uint32_t)i;
			return GAS_OK;
		}
	}
	c->streams.push_back(si);
	*out_stream = (uint32_t)c->streams.size() - 1;
	return GAS_OK;
}

int gas_stream_destroy(gas_ctx *c, uint32_t stream) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (stream >= c->streams.size() || !c->streams[stream].d_pcm) {
		return GAS_ERR_BAD_SLOT;
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	for (gas_cursor &cur : c->h_cursors) {
		if (cur.pcm == c->streams[stream].d_pcm) {
			return GAS_ERR_INVALID_ARGUMENT; // still bound to a playback
		}
	}
	c->mem.drop(c->streams[stream].d_pcm);
	c->streams[stream] = gas_ctx::StreamInfo{};
	return GAS_OK;
}

int gas_stream_get_info(gas_ctx *c, uint32_t stream, uint64_t *out_frames, uint32_t *out_channels, int *out_format) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (stream >= c->streams.size() || !c->streams[stream].d_pcm) {
		return GAS_ERR_BAD_SLOT;
	}
	if (out_frames) {
		*out_frames = c->streams[stream].frames;
	}
	if (out_channels) {
		*out_channels = c->streams[stream].channels;
	}
	if (out_format) {
		*out_format = (int)c->streams[stream].format;
	}
	return GAS_OK;
}

int gas_stream_positions(gas_ctx *c, uint32_t n, uint64_t *out_frames) {
	if (!c || (n > 0 && !out_frames)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (n != c->stream_slots_host.size()) {
		return GAS_ERR_INVALID_ARGUMENT; // not the list of the last stream callback (gas_process_block_streams or gas_process_block_streams_buses)
	}
	// The compact row mirror holds the positions while the list is cached; a block boundary that applied deferred
	// frees has folded it back into the per-slot cursors (stream_rows_sync_back) and emptied it.
	const bool rows_live = c->stream_rows.size() == n;
	for (uint32_t i = 0; i < n; i++) {
		const gas_cursor &cur = c->h_cursors[c->stream_slots_host[i]];
		if (!cur.pcm) {
			out_frames[i] = 0;
		} else if (rows_live) {
			const gas_ctx::StreamRow &r = c->stream_rows[i];
			out_frames[i] = r.resampled ? (r.fp_pos >> 16) : r.looped ? r.pos : cur.frames - r.remaining;
		} else {
			out_frames[i] = cur.resampled ? (cur.fp_pos >> 16) : cur.pos;
		}
		if (cur.pcm && cur.loop_mode) { // the stream frame taken next, m(frames consumed)
			out_frames[i] = gas_loop_map(out_frames[i], cur.loop_begin, cur.loop_len, cur.loop_mode);
		}
	}
	return GAS_OK;
}

int gas_stream_set_resampled(gas_ctx *c, uint32_t stream, int on) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (stream >= c->streams.size() || !c->streams[stream].d_pcm) {
		return GAS_ERR_BAD_SLOT;
	}
	for (const gas_cursor &cur : c->h_cursors) {
		if (cur.pcm == c->streams[stream].d_pcm) {
			return GAS_ERR_INVALID_ARGUMENT; // the playback class is chosen before playbacks are bound
		}
	}
	c->streams[stream].resampled = on != 0;
	return GAS_OK;
}

int gas_stream_set_loop(gas_ctx *c, uint32_t stream, int mode, uint64_t loop_begin, uint64_t loop_end) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (stream >= c->streams.size() || !c->streams[stream].d_pcm) {
		return GAS_ERR_BAD_SLOT;
	}
	gas_ctx::StreamInfo &si = c->streams[stream];
	for (const gas_cursor &cur : c->h_cursors) {
		if (cur.pcm == si.d_pcm) {
			return GAS_ERR_INVALID_ARGUMENT; // the loop is chosen before playbacks are bound
		}
	}
	if (mode == GAS_LOOP_DISABLED) {
		si.loop_mode = 0;
		si.loop_begin = si.loop_end = 0;
		return GAS_OK;
	}
	if (mode != GAS_LOOP_FORWARD && mode != GAS_LOOP_PINGPONG) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	const uint64_t end = loop_end == 0 ? si.frames : loop_end;
	if (loop_begin >= end || end > si.frames || end - loop_begin >= (1ull << 31)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	si.loop_mode = (uint32_t)mode;
	si.loop_begin = loop_begin;
	si.loop_end = end;
	return GAS_OK;
}

int gas_stream_get_loop(gas_ctx *c, uint32_t stream, int *out_mode, uint64_t *out_begin, uint64_t *out_end) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (stream >= c->streams.size() || !c->streams[stream].d_pcm) {
		return GAS_ERR_BAD_SLOT;
	}
	if (out_mode) {
		*out_mode = (int)c->streams[stream].loop_mode;
	}
	if (out_begin) {
		*out_begin = c->streams[stream].loop_begin;
	}
	if (out_end) {
		*out_end = c->streams[stream].loop_end;
	}
	return GAS_OK;
}

int gas_source_bind_stream(gas_ctx *c, uint32_t slot, uint32_t stream, uint64_t start_frame) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (slot >= c->cfg.max_sources || !c->slots[slot].used || stream >= c->streams.size() || !c->streams[stream].d_pcm) {
		return GAS_ERR_BAD_SLOT;
	}
	stream_rows_sync_back_fwd(c);
	c->stream_groups_gen = UINT64_MAX;
	feed_drop(c, slot); // gas_source_feed_rows: the stream supplies the windows from here on
	const gas_ctx::StreamInfo &si = c->streams[stream];
	gas_cursor cur{};
	cur.pcm = si.d_pcm;
	cur.frames = si.frames;
	cur.pos = start_frame < si.frames ? start_frame : si.frames;
	if (si.loop_mode) { // a position on the unrolled timeline: not clamped
		cur.pos = start_frame;
		cur.loop_begin = si.loop_begin;
		cur.loop_len = (uint32_t)(si.loop_end - si.loop_begin);
		cur.loop_mode = si.loop_mode;
	}
	cur.start = cur.pos;
	cur.format_channels = (si.format << 8) | si.channels;
	cur.has_frames = 1;
	cur.resampled = si.resampled ? 1 : 0;
	cur.fp_pos = cur.pos << 16; // [ENGINE] begin_resample: mix_offset = 0, zeroed interpolation history
	c->h_cursors[slot] = cur;
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipMemcpyAsync(c->d_cursors + slot, &c->h_cursors[slot], sizeof(gas_cursor), hipMemcpyHostToDevice, c->stream));
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	if (c->slots[slot].draining) {
		c->slots[slot].draining = 0;
		c->cached_n = UINT32_MAX;
	}
	return GAS_OK;
}

} // extern "C"

namespace {
// Write the compact per-row mirror of the cached stream list back into the per-slot cursors.
void stream_rows_sync_back(gas_ctx *c) {
	for (size_t i = 0; i < c->stream_rows.size(); i++) {
		gas_cursor &cur = c->h_cursors[c->stream_slots_host[i]];
		const gas_ctx::StreamRow &r = c->stream_rows[i];
		if (cur.pcm) {
			cur.pos = r.looped ? r.pos : cur.frames - r.remaining;
		}
		if (r.resampled) {
			cur.fp_pos = r.fp_pos;
		}
		cur.has_frames = r.has_frames;
	}
	c->stream_rows.clear();
}

inline size_t feed_header_bytes(const gas_ctx *c) {
	return ((size_t)c->cfg.max_sources * sizeof(uint32_t) + 15) & ~(size_t)15;
}

// Where the next `bytes` of rows go in the feed table.  The table is allocated once, at the first feed: the header and
// two halves of max_sources float32 stereo rows each.  Rows are appended in the current half.  When it is full -- rows
// that were replaced, or fed while no callback ran, leave holes -- the pending rows this call does not replace (those
// without its stamp) move to the front of the other half and the new rows follow them: together at most max_sources
// rows, so they fit.  Everything is a copy in the context's stream order from one half into the other: no allocation and
// no wait on the audio thread.  Nothing is committed here: feed_moved holds the moved rows' new words, and the caller
// switches halves once its own copy is enqueued.
int feed_place(gas_ctx *c, size_t bytes, size_t &at, bool &switched) {
	const size_t hdr = feed_header_bytes(c), half = (size_t)c->cfg.max_sources * c->cfg.frames * sizeof(gas_audio_frame);
	if (!c->d_feed) {
		if (alloc_once(c, c->h_feed_entry, c->cfg.max_sources, Mem::PINNED) != hipSuccess) {
			return GAS_ERR_OUT_OF_MEMORY;
		}
		if (!c->feed_entry_ev) {
			GAS_HIP(c, c->mem.make_event(c->feed_entry_ev, hipEventDisableTiming));
		}
		if (c->mem.alloc(c->d_feed, hdr + 2 * half) != hipSuccess) {
			return GAS_ERR_OUT_OF_MEMORY;
		}
		c->feed_used = 0;
	}
	if (c->feed_used < hdr) { // emptied by a callback: start over
		c->feed_used = hdr;
		c->feed_side = 0;
	}
	c->feed_moved.clear();
	switched = false;
	if (c->feed_used + bytes <= hdr + (c->feed_side + 1) * half) {
		at = c->feed_used;
		return GAS_OK;
	}
	switched = true;
	const uint32_t F = c->cfg.frames;
	size_t off = hdr + (1 - c->feed_side) * half;
	for (uint32_t s : c->feed_slots) {
		if (c->stamp.has(s)) {
			continue; // this call replaces it
		}
		const uint32_t w = c->feed_word[s];
		const size_t rb = gas_feed_row_bytes(w, F);
		GAS_HIP(c, hipMemcpyAsync(c->d_feed + off, c->d_feed + gas_feed_offset(w), rb, hipMemcpyDeviceToDevice, c->stream));
		c->feed_moved.push_back(s);
		c->feed_moved.push_back(gas_feed_word(off, (w & 2u) ? GAS_PCM_F32 : GAS_PCM_S16, (w & 1u) + 1u));
		off += rb;
	}
	at = off;
	return GAS_OK;
}

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

// A failed callback leaves a zeroed mix in host memory (the reference's ERR_FAIL paths, audio_spatializer.cpp:335-343);
// device memory is left as it is.
int fail_out(int code, int mem, gas_audio_frame *out, size_t out_bytes) {
	if (mem == GAS_MEM_HOST) {
		std::memset(out, 0, out_bytes);
	}
	return code;
}
} // namespace

extern "C" {

// The bodies of gas_process_block and gas_process_block_buses, behind their argument checks; the stream entries call
// them with a fused source.
static int process_block(gas_ctx *c, const RowSource &src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, float *peaks, int mem);
static int process_block_buses(gas_ctx *c, const RowSource &src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, uint32_t n_buses, float *peaks, int mem);

// Both stream entries: validation, the host mirror of the cursor arithmetic, the same_list steady state, the sampler
// launches and the choice of the fused form.  !buses: gas_process_block_streams (one mix, out [C][frames], n_buses unused); buses:
// gas_process_block_streams_buses (out [n_buses][C][frames], the device path of gas_process_block_buses over the windows).
static int process_block_streams_common(gas_ctx *c, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, uint32_t n_buses, bool buses, float *peaks, uint8_t *has_frames, int mem) {
	if (!c || !out || (n > 0 && !slots) || n > c->cfg.max_sources || (mem != GAS_MEM_HOST && mem != GAS_MEM_DEVICE)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (buses && (n_buses < 1 || n_buses > GAS_MAX_BUSES)) {
		if (mem == GAS_MEM_HOST) { // as much of `out` as a legal call could name
			std::memset(out, 0, (size_t)(n_buses < GAS_MAX_BUSES ? n_buses : GAS_MAX_BUSES) * c->cfg.channel_count * c->cfg.frames * sizeof(gas_audio_frame));
		}
		return GAS_ERR_INVALID_ARGUMENT;
	}
	GAS_TRY(flush_deferred(c)); // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
	const uint32_t F = c->cfg.frames, C = c->cfg.channel_count;
	const size_t out_bytes = (size_t)(buses ? n_buses : 1u) * C * F * sizeof(gas_audio_frame);
	const auto fail = [&](int code) { return fail_out(code, mem, out, out_bytes); };
	if (frames != F) {
		return fail(GAS_ERR_FRAME_COUNT);
	}
	if (hipSetDevice(c->cfg.device) != hipSuccess) {
		return fail(GAS_ERR_NO_DEVICE);
	}
	// Steady state: same slot list as the previous stream callback, launch groups still cached, no parameter or
	// binding change since -> skip validation and work on the compact row mirror.
	// (The staged bus form regroups on every call and leaves no cached groups behind: its list stays "the same" without them.)
	adopt_frees(c);
	bool same_list = c->pending_free.empty() /* a deferred free re-sorts the groups */ && c->stream_rows.size() == n && (c->cached_n == n || (buses && c->stream_bus_staged)) && c->stream_last_buses == buses && c->stream_groups_gen == c->groups_gen && !c->stream_params_touched && c->stream_slots_host.size() == n && (n == 0 || std::memcmp(c->stream_slots_host.data(), slots, (size_t)n * sizeof(uint32_t)) == 0);
	if (!same_list) {
		stream_rows_sync_back(c);
		for (uint32_t i = 0; i < n; i++) {
			if (!live(c, slots[i])) {
				return fail(GAS_ERR_BAD_SLOT);
			}
			const float pitch = c->slots[slots[i]].has_params ? c->h_params[slots[i]].pitch_scale : 1.0f;
			if (!c->h_cursors[slots[i]].pcm) {
				// bound to no stream: a fed row or silence.  pitch_scale is the sampler's input, and whoever decodes this
				// playback has applied it already (the host layer hands it to the playback's mix callback), as for the
				// rows of gas_process_block
			} else if (c->h_cursors[slots[i]].resampled) {
				if (!(pitch >= 0.0f && pitch < 32768.0f)) {
					return fail(GAS_ERR_INVALID_ARGUMENT);
				}
			} else if (pitch != 1.0f && pitch != 0.0f) {
				return fail(GAS_ERR_UNSUPPORTED_CHAIN); // a non-resampled playback class (gas_stream_set_resampled is off)
			}
		}
		// Everything gas_process_block could still reject is checked BEFORE a cursor moves: the reference consumes a
		// playback's frames only when it mixes them (audio_spatializer.cpp:378), so a failed callback must leave
		// the playback cursors (host mirror and device) where they were.
		c->stamp.next();
		for (uint32_t i = 0; i < n; i++) {
			const SlotInfo &si = c->slots[slots[i]];
			if (!si.has_params) {
				return fail(GAS_ERR_NO_PARAMS);
			}
			if (c->stamp.seen(slots[i])) {
				return fail(GAS_ERR_INVALID_ARGUMENT); // one playback twice in a callback
			}
			const bool wants_hrtf = si.group == G_FX_HRTF || si.group == G_FX_ER_HRTF || (si.group == G_FX_GENERIC && chain_has(si.chain_sig, GAS_FX_HRTF));
			if (wants_hrtf && c->tab.spec == nullptr) {
				return fail(GAS_ERR_NO_HRTF);
			}
		}
		if (buses && bus_list_form(c, slots, n) == BUS_LIST_NEITHER) {
			return fail(GAS_ERR_UNSUPPORTED_CHAIN); // process_block_buses would, after the cursors have moved
		}
		c->stream_last_buses = buses;
		c->stream_bus_staged = false;
		c->stream_params_touched = false;
		c->stream_slots_host.assign(slots, slots + n);
		c->stream_rows.resize(n);
		c->stream_all_hrtf = n > 0;
		c->stream_any_resampled = false;
		c->stream_any_looped = false;
		c->stream_any_adpcm = false;
		c->stream_any_qoa = false;
		for (uint32_t i = 0; i < n; i++) {
			const gas_cursor &cur = c->h_cursors[slots[i]];
			c->stream_any_adpcm = c->stream_any_adpcm || (cur.pcm && (cur.format_channels >> 8) == GAS_PCM_IMA_ADPCM);
			c->stream_any_qoa = c->stream_any_qoa || (cur.pcm && (cur.format_channels >> 8) == GAS_PCM_QOA);
			gas_ctx::StreamRow &r = c->stream_rows[i];
			r.remaining = cur.pcm && cur.frames > cur.pos ? cur.frames - cur.pos : 0;
			r.has_frames = cur.pcm ? cur.has_frames : 0;
			r.resampled = cur.pcm ? cur.resampled : 0;
			r.looped = cur.pcm && cur.loop_mode ? 1 : 0;
			r.pos = cur.pos;
			c->stream_any_looped = c->stream_any_looped || r.looped;
			r.inc = 65536;
			if (r.resampled) {
				// [ENGINE] mix_increment = uint64((stream_rate * rate_scale / mix_rate) * FP_LEN), stream at the mix rate
				const float pitch = c->slots[slots[i]].has_params ? c->h_params[slots[i]].pitch_scale : 1.0f;
				r.inc = (uint32_t)(uint64_t)(((double)(c->cfg.mix_rate * pitch) / (double)c->cfg.mix_rate) * 65536.0);
				r.fp_pos = cur.fp_pos;
				r.end_fp = cur.frames << 16;
				c->stream_any_resampled = true;
			}
			c->h_stream_inc[i] = r.inc;
			c->stream_all_hrtf = c->stream_all_hrtf && c->slots[slots[i]].group == G_FX_HRTF;
		}
		if (c->stream_any_resampled) {
			hipError_t e = hipMemcpyAsync(c->d_stream_inc, c->h_stream_inc, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
			if (e == hipSuccess) {
				e = hipStreamSynchronize(c->stream); // the pinned staging array is rewritten by the next list
			}
			if (e != hipSuccess) {
				c->last_err = hipGetErrorString(e);
				return fail(GAS_ERR_DEVICE);
			}
		}
		if (n > 0) {
			hipError_t e = hipMemcpyAsync(c->d_stream_slots, c->stream_slots_host.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
			if (e != hipSuccess) {
				c->last_err = hipGetErrorString(e);
				return fail(GAS_ERR_DEVICE);
			}
		}
	}
	// host mirror of the cursor arithmetic: which playbacks end inside this callback (audio_spatializer.cpp:380,398)
	bool draining_changed = false;
	// gas_source_feed_rows: which entries take a fed row is this callback's matter alone, read from the pending rows and
	// never from the cached list -- the steady state above holds whatever is fed, not fed, or fed again under it.
	const bool feed_pending = !c->feed_slots.empty();
	bool any_fed = false;
	if (feed_pending) {
		c->feed_entry.assign(n, GAS_FEED_NONE);
	}
	for (uint32_t i = 0; i < n; i++) {
		gas_ctx::StreamRow &r = c->stream_rows[i];
		if (feed_pending && c->feed_word[slots[i]] != GAS_FEED_NONE) { // a live playback without a cursor: nothing moves, nothing ends
			c->feed_entry[i] = c->feed_word[slots[i]];
			any_fed = true;
			r.draining_marked = 0; // the next callback that finds it unfed marks it draining again
			if (has_frames) {
				has_frames[i] = 1;
			}
			continue;
		}
		if (r.has_frames && r.resampled) { // same arithmetic as k_sample_sources' resampled branch
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
	if (draining_changed) {
		c->cached_n = UINT32_MAX;
		same_list = false;
	}
	if (any_fed && c->feed_entry != c->feed_entry_dev) { // the list or the fed set changed: the table's header follows
		hipError_t e = hipEventSynchronize(c->feed_entry_ev); // the previous header has left the pinned words: a wait only while that upload is still queued
		if (e == hipSuccess) {
			std::memcpy(c->h_feed_entry, c->feed_entry.data(), (size_t)n * sizeof(uint32_t));
			e = hipMemcpyAsync(c->d_feed, c->h_feed_entry, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
		}
		if (e == hipSuccess) {
			e = hipEventRecord(c->feed_entry_ev, c->stream);
		}
		if (e != hipSuccess) {
			c->feed_entry_dev.clear();
			c->last_err = hipGetErrorString(e);
			return fail(GAS_ERR_DEVICE);
		}
		c->feed_entry_dev = c->feed_entry;
	}
	if (feed_pending) { // one feed serves one callback; rows of slots the list does not name go with it
		for (uint32_t s : c->feed_slots) {
			c->feed_word[s] = GAS_FEED_NONE;
		}
		c->feed_slots.clear();
		c->feed_used = 0;
	}
	const uint8_t *feed = any_fed ? c->d_feed : nullptr;
	// rows for this callback live in the library's staging buffer (not needed when k_hrtf_ols samples the
	// streams itself: every playback a plain [HRTF] chain)
	// (GAS_FLAG_HRTF_BLEND_FADE: the stream-sampling form has no registers left for the fade, DESIGN.md 3.4 -- rows first)
	// (gas_stream_set_loop: the cross-fade form has no registers left for the looped branch either, DESIGN.md 3.4 -- rows first)
	const bool loops_fused = !c->stream_any_looped || (c->cfg.flags & GAS_FLAG_HRTF_CROSSFADE) == 0;
	// (GAS_PCM_IMA_ADPCM, GAS_PCM_QOA: the fused prologues read uncompressed frames only -- rows first, like a resampled playback)
	// (buses: the fused form is k_hrtf_uni<SRC_PCM, BUS2>, which gas_process_block_buses picks on a one-pair context without a k_hrtf_ols-only mode)
	const bool bus_fusable = !buses || (C == 1 && uni_ok(c) && gas_hrtf_uni_waves() == 8);
	// (gas_source_feed_rows: k_hrtf_uni<SRC_PCM> and k_hrtf_uni<SRC_PCM, BUS2> take fed entries; the k_hrtf_ols stream-sampling forms -- cross-fade, direction runs / order, interpolation contexts -- have no registers left for them, DESIGN.md 3.4 -- rows first)
	const bool fed_fusable = !any_fed || uni_ok(c);
	const bool all_hrtf = c->stream_all_hrtf && !c->stream_any_resampled && !c->stream_any_adpcm && !c->stream_any_qoa && !fade_on(c) && loops_fused && !c->stream_rows_first && bus_fusable && fed_fusable; // the fused prologue samples plain playbacks only
	c->stream_last_fused = all_hrtf;
	if (!all_hrtf) {
		if (ensure_src(c, (size_t)n * F) != hipSuccess) {
			return fail(GAS_ERR_OUT_OF_MEMORY);
		}
		if (n > 0) {
			hipError_t e = gas_launch_sample_sources(c->stream, c->d_cursors, c->d_stream_slots, n, F, c->d_fade_env, c->d_src, c->stream_any_resampled ? c->d_stream_inc : nullptr, feed);
			if (e == hipSuccess && c->stream_any_adpcm) {
				e = gas_launch_sample_adpcm(c->stream, c->d_cursors, c->d_stream_slots, n, F, c->d_fade_env, c->d_src, c->stream_any_resampled ? c->d_stream_inc : nullptr, c->adpcm_span);
			}
			if (e == hipSuccess && c->stream_any_qoa) {
				e = gas_launch_sample_qoa(c->stream, c->d_cursors, c->d_stream_slots, n, F, c->d_fade_env, c->d_src, c->stream_any_resampled ? c->d_stream_inc : nullptr, c->qoa_span);
			}
			if (e != hipSuccess) {
				c->last_err = hipGetErrorString(e);
				return fail(GAS_ERR_DEVICE);
			}
		}
	}
	RowSource rows; // fused: no float rows, the HRTF launch samples the bound streams (and the fed rows) itself
	if (all_hrtf) {
		rows.cursors = c->d_cursors;
		rows.feed = feed;
	} else {
		rows.rows = c->d_src;
	}
	// host outputs: the device path into the library's buffers, one copy back
	gas_audio_frame *d_out = out;
	float *d_pk = peaks;
	if (mem == GAS_MEM_HOST) {
		const int rcs = stage_host(c, nullptr, n, buses, d_out, d_pk);
		if (rcs != GAS_OK) {
			return fail(rcs);
		}
	}
	int rc = GAS_OK;
	if (buses) {
		// gas_process_block_buses reuses a list only for its 3D-mix and fused [HRTF] forms; the staged form needs it every time
		const bool reuse = same_list && n > 0 && c->cached_n == n && c->bus_form_cached != 0 && c->bus_form_groups_gen == c->groups_gen;
		rc = process_block_buses(c, rows, reuse ? nullptr : slots, n, F, d_out, n_buses, d_pk, GAS_MEM_DEVICE);
		c->stream_bus_staged = rc == GAS_OK && n > 0 && c->cached_n != n; // ran staged: nothing cached to compare with next time
	} else {
		rc = process_block(c, rows, same_list ? nullptr : slots, n, F, d_out, d_pk, GAS_MEM_DEVICE);
	}
	c->stream_groups_gen = rc == GAS_OK ? c->groups_gen : UINT64_MAX;
	if (rc == GAS_OK && !buses && mem == GAS_MEM_HOST) {
		rc = join_outputs(c);
	}
	if (rc != GAS_OK) {
		return fail(rc);
	}
	if (mem == GAS_MEM_DEVICE) {
		return GAS_OK;
	}
	const hipError_t e = copy_back(c, out, d_out, out_bytes, peaks, n);
	if (e != hipSuccess) {
		c->last_err = hipGetErrorString(e);
		return fail(GAS_ERR_DEVICE);
	}
	return GAS_OK;
}

int gas_process_block_streams(gas_ctx *c, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, float *peaks, uint8_t *has_frames, int mem) {
	return process_block_streams_common(c, slots, n, frames, out, 0, false, peaks, has_frames, mem);
}

int gas_process_block_streams_buses(gas_ctx *c, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, uint32_t n_buses, float *peaks, uint8_t *has_frames, int mem) {
	return process_block_streams_common(c, slots, n, frames, out, n_buses, true, peaks, has_frames, mem);
}

int gas_stream_last_fused(gas_ctx *c) {
	return c ? (c->stream_last_fused ? 1 : 0) : GAS_ERR_INVALID_ARGUMENT;
}

int gas_source_feed_rows(gas_ctx *c, const uint32_t *slots, const void *rows, int format, uint32_t channels, uint32_t n, uint32_t frames, int mem) {
	if (!c || (n > 0 && (!slots || !rows)) || n > c->cfg.max_sources || (format != GAS_PCM_S16 && format != GAS_PCM_F32) || (channels != 1 && channels != 2) || (mem != GAS_MEM_HOST && mem != GAS_MEM_DEVICE)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	const uint32_t F = c->cfg.frames;
	if (frames != F) {
		return GAS_ERR_FRAME_COUNT;
	}
	GAS_TRY(flush_deferred(c)); // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
	// everything is checked before anything is taken
	c->stamp.next();
	{
		std::lock_guard<std::mutex> alloc_lk(c->alloc_mu); // pending_free is set by gas_source_free on any thread
		for (uint32_t i = 0; i < n; i++) {
			if (!live(c, slots[i]) || c->slots[slots[i]].pending_free) {
				return GAS_ERR_BAD_SLOT;
			}
		}
	}
	for (uint32_t i = 0; i < n; i++) {
		if (c->h_cursors[slots[i]].pcm) {
			return GAS_ERR_INVALID_ARGUMENT; // bound to a stream: the sampler supplies its windows
		}
		if (c->stamp.seen(slots[i])) {
			return GAS_ERR_INVALID_ARGUMENT; // one playback twice in a call
		}
	}
	if (n == 0) {
		return GAS_OK;
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	const size_t row_bytes = (size_t)F * (format == GAS_PCM_F32 ? 4u : 2u) * channels; // a multiple of 256: frames % 128 == 0
	const size_t bytes = (size_t)n * row_bytes;
	if (mem == GAS_MEM_HOST && bytes > c->h_feed_cap) { // grows to the largest call: not in the steady state
		if (c->feed_ev) {
			GAS_HIP(c, hipEventSynchronize(c->feed_ev));
		} else {
			GAS_HIP(c, c->mem.make_event(c->feed_ev, hipEventDisableTiming));
		}
		if (c->mem.grow(c->h_feed, c->h_feed_cap, bytes, 1, Mem::PINNED) != hipSuccess) {
			return GAS_ERR_OUT_OF_MEMORY;
		}
	}
	size_t at = 0;
	bool switched = false;
	const int rcp = feed_place(c, bytes, at, switched);
	if (rcp != GAS_OK) {
		return rcp;
	}
	uint8_t *dst = c->d_feed + at;
	const int rcc = [&]() -> int {
		if (mem == GAS_MEM_DEVICE) {
			const int rcj = join_outputs(c); // GAS_FLAG_PIPELINED_MIX: `rows` may be an earlier callback's out, still a pending sum
			if (rcj != GAS_OK) {
				return rcj;
			}
			GAS_HIP(c, hipMemcpyAsync(dst, rows, bytes, hipMemcpyDeviceToDevice, c->stream));
			return GAS_OK;
		}
		GAS_HIP(c, hipEventSynchronize(c->feed_ev)); // the previous upload has left the staging: a wait only while it is still queued
		std::memcpy(c->h_feed, rows, bytes);
		GAS_HIP(c, hipMemcpyAsync(dst, c->h_feed, bytes, hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, hipEventRecord(c->feed_ev, c->stream));
		return GAS_OK;
	}();
	if (rcc != GAS_OK) {
		return rcc; // nothing committed: every pending row is still where its word says
	}
	if (switched) {
		c->feed_side = 1 - c->feed_side;
		for (size_t k = 0; k + 1 < c->feed_moved.size(); k += 2) {
			c->feed_word[c->feed_moved[k]] = c->feed_moved[k + 1];
		}
	}
	for (uint32_t i = 0; i < n; i++) {
		if (c->feed_word[slots[i]] == GAS_FEED_NONE) {
			c->feed_slots.push_back(slots[i]);
		} // else: replaces the row fed before; its bytes lie idle until the table is emptied
		c->feed_word[slots[i]] = gas_feed_word(at + (size_t)i * row_bytes, format, channels);
	}
	c->feed_used = at + bytes;
	return GAS_OK;
}

int gas_hrtf_load(gas_ctx *c, const float *hrir, uint32_t dirs, uint32_t taps) {
	if (!c || !hrir || dirs == 0 || taps == 0 || taps > GAS_HRTF_TAPS) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	{ // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
		const int rcd = flush_deferred(c);
		if (rcd != GAS_OK) {
			return rcd;
		}
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	c->mem.drop(c->tab.spec);
	c->tab.dirs = 0;
	Mem tmp; // frees d_hrir on every way out
	float *d_hrir = nullptr;
	const size_t floats = (size_t)dirs * 2 * taps;
	GAS_HIP(c, tmp.alloc(d_hrir, floats));
	GAS_HIP(c, hipMemcpyAsync(d_hrir, hrir, floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
	GAS_HIP(c, c->mem.alloc(c->tab.spec, (size_t)dirs * 4 * 64)); // bins 0..255, Hermitian half
	GAS_HIP(c, gas_launch_hrtf_table(c->stream, d_hrir, dirs, taps, c->d_tw, c->tab.spec));
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	c->tab.dirs = dirs;
	c->params_gen++;
	return GAS_OK;
}

int gas_hrtf_load_positions(gas_ctx *c, const float *positions, const float *hrir, uint32_t m, uint32_t taps, uint32_t az_steps, uint32_t el_steps, int interpolation, float *out_hrir) {
	if (!c || !positions || !hrir || m == 0 || taps == 0 || taps > GAS_HRTF_TAPS || az_steps == 0 || el_steps == 0 || (uint64_t)az_steps * el_steps > (1u << 20) || (interpolation != 0 && interpolation != 1)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	const uint32_t dirs = az_steps * el_steps;
	std::vector<float> grid((size_t)dirs * 2 * GAS_HRTF_TAPS);
	{
		Mem tmp; // frees the three on every way out of the block
		float *d_pos = nullptr, *d_in = nullptr, *d_grid = nullptr;
		GAS_HIP(c, tmp.alloc(d_pos, (size_t)m * 2));
		GAS_HIP(c, tmp.alloc(d_in, (size_t)m * 2 * taps));
		GAS_HIP(c, tmp.alloc(d_grid, grid.size()));
		GAS_HIP(c, hipMemcpyAsync(d_pos, positions, (size_t)m * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, hipMemcpyAsync(d_in, hrir, (size_t)m * 2 * taps * sizeof(float), hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, gas_launch_hrtf_regrid(c->stream, d_pos, d_in, m, taps, az_steps, el_steps, interpolation, d_grid));
		GAS_HIP(c, hipMemcpyAsync(grid.data(), d_grid, grid.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
		GAS_HIP(c, hipStreamSynchronize(c->stream));
	}
	if (out_hrir) {
		std::memcpy(out_hrir, grid.data(), grid.size() * sizeof(float));
	}
	return gas_hrtf_load(c, grid.data(), dirs, GAS_HRTF_TAPS);
}

int gas_process_block(gas_ctx *c, const gas_audio_frame *src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, float *peaks, int mem) {
	if (!c || !out || (mem != GAS_MEM_HOST && mem != GAS_MEM_DEVICE) || (n > 0 && !src) || n > c->cfg.max_sources) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	RowSource rows;
	rows.rows = src;
	return process_block(c, rows, slots, n, frames, out, peaks, mem);
}

static int process_block(gas_ctx *c, const RowSource &src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, float *peaks, int mem) {
	const uint32_t F = c->cfg.frames, C = c->cfg.channel_count;
	const size_t out_bytes = (size_t)C * F * sizeof(gas_audio_frame);
	int rc = GAS_OK;
	const auto fail = [&](int code) { return fail_out(code, mem, out, out_bytes); };
	if (frames != F) {
		return fail(GAS_ERR_FRAME_COUNT);
	}
	if (hipSetDevice(c->cfg.device) != hipSuccess) {
		return fail(GAS_ERR_NO_DEVICE);
	}
	adopt_frees(c);
	if (!c->deferred.empty()) { // GAS_FLAG_BATCHED_LAUNCH: do the waiting callbacks still see what they were recorded with?
		bool host_dirty = false;
		{
			std::lock_guard<std::mutex> lk(c->params_mu);
			host_dirty = !c->dirty_list.empty() || !c->fx[FX_BASIC].dirty_list.empty() || !c->blend_dirty_list.empty();
		}
		const bool keep = mem == GAS_MEM_DEVICE && !slots && n == c->deferred_n && c->pending_free.empty() && c->groups_gen == c->deferred_groups_gen && !host_dirty;
		if (!keep) {
			rc = flush_deferred(c);
			if (rc != GAS_OK) {
				return fail(rc);
			}
		}
	}
	if (c->pending_params && (slots || n == 0 || c->cached_n != n || !c->pending_free.empty())) {
		rc = flush_pending_params(c); // the list may change: scatter with the mapping it was published for
		if (rc != GAS_OK) {
			return fail(rc);
		}
	}
	apply_pending_frees(c);
	if (slots || n == 0) { // an empty callback needs no list
		rc = build_groups(c, slots, n, false);
		if (rc != GAS_OK) {
			c->cached_n = UINT32_MAX;
			return fail(rc);
		}
	} else if (c->cached_n != n) {
		return fail(GAS_ERR_INVALID_ARGUMENT);
	}
	if (needs_hrtf(c)) {
		return fail(GAS_ERR_NO_HRTF);
	}
	const uint64_t pgen = c->params_gen.load(); // read before the snapshot: a publish racing with it re-sorts next time
	rc = flush_params(c); // one snapshot per callback (audio_spatializer.cpp:328)
	if (rc != GAS_OK) {
		return fail(rc);
	}
	if (c->order_groups_gen != c->groups_gen || c->order_params_gen != pgen) {
		std::memset(c->order_ok, 0, sizeof(c->order_ok));
		c->order_groups_gen = c->groups_gen;
		c->order_params_gen = pgen;
	}

	RowSource d_src = src;
	gas_audio_frame *d_out = out;
	float *d_peaks = peaks ? peaks : c->d_peaks;
	if (mem == GAS_MEM_HOST) {
		rc = stage_host(c, src.rows, n, false, d_out, d_peaks);
		if (rc != GAS_OK) {
			return fail(rc);
		}
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
			rc = flush_pending_params(c);
			if (rc != GAS_OK) {
				return fail(rc);
			}
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
		if (c->deferred.size() >= depth) {
			rc = flush_deferred(c);
			return rc == GAS_OK ? GAS_OK : fail(rc);
		}
		return GAS_OK;
	}
	if (!c->deferred.empty()) {
		rc = flush_deferred(c);
		if (rc != GAS_OK) {
			return fail(rc);
		}
	}
	RunArgs a = own_list(c, d_src, n, d_out, d_peaks);
	a.channel_count = C;
	a.use_order = true;
	a.pipelined = mem == GAS_MEM_DEVICE;
	a.fresh = fresh;
	rc = run_groups(c, a);
	if (rc != GAS_OK) {
		return fail(rc);
	}
	if (mem == GAS_MEM_HOST) {
		const hipError_t e = copy_back(c, out, c->d_out, out_bytes, peaks, n);
		if (e != hipSuccess) {
			c->last_err = hipGetErrorString(e);
			return fail(GAS_ERR_DEVICE);
		}
	}
	return GAS_OK;
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

// AudioSpatializer3D's buses in one launch: the mix_channel kernel with per-source weights per bus, its partial
// planes summed by the ordinary deterministic reduce (bus-major: plane b * C + c).
int gas_process_block_buses(gas_ctx *c, const gas_audio_frame *src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, uint32_t n_buses, float *peaks, int mem) {
	// slots == NULL: the list (and grouping) of the previous call, like gas_process_block -- for the two forms whose
	// grouping is the ordinary one (3D mix, fused [HRTF])
	if (!c || !out || (mem != GAS_MEM_HOST && mem != GAS_MEM_DEVICE) || (n > 0 && !src) || n > c->cfg.max_sources || n_buses < 1 || n_buses > GAS_MAX_BUSES) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	RowSource rows;
	rows.rows = src;
	return process_block_buses(c, rows, slots, n, frames, out, n_buses, peaks, mem);
}

static int process_block_buses(gas_ctx *c, const RowSource &src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, uint32_t n_buses, float *peaks, int mem) {
	adopt_frees(c);
	if (n > 0 && !slots && (c->cached_n != n || c->bus_form_cached == 0 || c->bus_form_groups_gen != c->groups_gen || !c->pending_free.empty())) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	GAS_TRY(flush_deferred(c)); // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
	const uint32_t F = c->cfg.frames, C = c->cfg.channel_count;
	const size_t out_bytes = (size_t)n_buses * C * F * sizeof(gas_audio_frame);
	const auto fail = [&](int code) { return fail_out(code, mem, out, out_bytes); };
	if (frames != F) {
		return fail(GAS_ERR_FRAME_COUNT);
	}
	if (hipSetDevice(c->cfg.device) != hipSuccess) {
		return fail(GAS_ERR_NO_DEVICE);
	}
	int rc = flush_pending_params(c);
	if (rc != GAS_OK) {
		return fail(rc);
	}
	apply_pending_frees(c);
	// Two forms: every source GAS_KIND_3D_MIX (the mix-channel buses of AudioSpatializer3D, fused in the biquad
	// kernels), or every source an effect chain (run staged: per-source rows, then mixed per bus) on a one-pair context.
	const bool reuse = n > 0 && !slots; // the cached form is 1 (3D mix) or 2 (fused [HRTF]) then
	const BusList form = reuse ? (c->bus_form_cached == 1 ? BUS_LIST_3D_MIX : BUS_LIST_PLAIN_HRTF) : bus_list_form(c, slots, n);
	const bool all_mix = form == BUS_LIST_3D_MIX;
	// [HRTF] sources onto one or two buses have a fused form (k_hrtf_uni<BUS2>: the second bus's spectra sums in LDS)
	// (three to six buses: one fused launch per pair of buses, the state committed by the last)
	const bool fused_hrtf = form == BUS_LIST_PLAIN_HRTF && uni_ok(c) && gas_hrtf_uni_waves() == 8;
	if (src.fused() && !(fused_hrtf && mem == GAS_MEM_DEVICE)) {
		return fail(GAS_ERR_INVALID_ARGUMENT); // gas_process_block_streams_buses hands over no rows: only the fused form can sample
	}
	const bool staged = (form == BUS_LIST_CHAINS || form == BUS_LIST_PLAIN_HRTF) && !fused_hrtf;
	if (reuse && staged) {
		return fail(GAS_ERR_INVALID_ARGUMENT); // the staged form regroups: it needs the list
	}
	if (!reuse) {
		rc = build_groups(c, slots, n, staged);
		c->cached_n = staged ? UINT32_MAX : c->cached_n; // the staged grouping is this call's only: a later list reuse must regroup
		if (rc != GAS_OK) {
			c->cached_n = UINT32_MAX;
			return fail(rc);
		}
	}
	c->bus_form_cached = staged ? 0 : (fused_hrtf ? 2 : (all_mix ? 1 : 0));
	c->bus_form_groups_gen = c->groups_gen;
	for (int gt = 0; gt < G_COUNT; gt++) {
		if (gt != (staged ? G_FX_GENERIC : (fused_hrtf ? G_FX_HRTF : G_3D_MIX)) && c->groups[gt].count > 0) {
			c->cached_n = UINT32_MAX;
			return fail(GAS_ERR_UNSUPPORTED_CHAIN);
		}
	}
	if ((staged || fused_hrtf) && needs_hrtf(c)) {
		return fail(GAS_ERR_NO_HRTF);
	}
	rc = join_outputs(c);
	if (rc == GAS_OK) {
		rc = flush_params(c);
	}
	if (rc != GAS_OK) {
		return fail(rc);
	}
	rc = [&]() -> int {
		// routes snapshot (latest wins), like the parameters
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
			const int rcg = run_groups(c, a);
			if (rcg != GAS_OK) {
				return rcg;
			}
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
			GAS_HIP(c, gas_launch_biquad_mix(c->stream, GAS_MODE_MIX_CHANNEL, ga, c->st, F, 0, C, c->cfg.mix_rate, c->d_bus_partials, 0, P, nullptr, ba));
		}
		if (!staged) {
			GAS_HIP(c, gas_launch_mix_reduce(c->stream, c->d_bus_partials, P, P ? P : 1, n_buses * C, F, d_out));
		}
		if (mem == GAS_MEM_HOST) {
			GAS_HIP(c, copy_back(c, out, c->d_bus_out, out_bytes, peaks, n));
		}
		return GAS_OK;
	}();
	return rc == GAS_OK ? GAS_OK : fail(rc);
}

static int process_one(gas_ctx *c, uint32_t slot, int channel, bool mix_channel, gas_audio_frame *out, const gas_audio_frame *src, int frame_count) {
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
	int rc = flush_pending_params(c);
	if (rc == GAS_OK) {
		rc = flush_params(c);
	}
	if (rc != GAS_OK) {
		return rc;
	}
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

int gas_process_frames_1(gas_ctx *c, uint32_t slot, gas_audio_frame *out, const gas_audio_frame *src, int frame_count) {
	return process_one(c, slot, 0, false, out, src, frame_count);
}

int gas_mix_channel_1(gas_ctx *c, uint32_t slot, int channel, gas_audio_frame *out, const gas_audio_frame *src, int frame_count) {
	return process_one(c, slot, channel, true, out, src, frame_count);
}

int gas_profile_enable(gas_ctx *c, int on) {
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
	if (on && c->ev.empty()) {
		std::vector<hipEvent_t> ev(PROFILE_EVENTS, nullptr);
		for (hipEvent_t &e : ev) {
			GAS_HIP(c, c->mem.make_event(e, hipEventDefault)); // a failure leaves c->ev empty and what exists to the owner
		}
		c->ev = std::move(ev);
	}
	if (on) {
		// An event pair around a launch reads the launch's span on the GPU timeline plus the cost of the second
		// marker.  Only the marker is calibrated away (an empty bracket, minimum of 16 tries): the dispatch ramp of
		// the kernel itself stays in, exactly as rocprofv3's kernel trace counts it (an empty kernel reads 3-4 us
		// there), so the two figures of one run agree and neither flatters the kernel.
		GAS_HIP(c, hipStreamSynchronize(c->stream));
		double best = 1e9;
		for (int i = 0; i < 16; i++) {
			GAS_HIP(c, hipEventRecord(c->ev[0], c->stream));
			GAS_HIP(c, hipEventRecord(c->ev[1], c->stream));
			GAS_HIP(c, hipEventSynchronize(c->ev[1]));
			float ms = 0.0f;
			GAS_HIP(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
			best = ms < best ? ms : best;
		}
		c->ev_overhead_ms = best;
	}
	c->profiling = on != 0;
	c->prof_every = on > 1 ? (uint32_t)on : 1; // on = N > 1: bracket every Nth callback only (the markers cost throughput)
	c->prof_tick = 0;
	return GAS_OK;
}

int gas_ctx_read_hrtf_order(gas_ctx *c, uint32_t *out, uint32_t n) {
	if (!c || !out) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	{ // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
		const int rcd = flush_deferred(c);
		if (rcd != GAS_OK) {
			return rcd;
		}
	}
	if (!c->d_order || !c->order_ok[G_FX_HRTF] || !c->last_uni_ordered || n > c->groups[G_FX_HRTF].count) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	GAS_HIP(c, hipMemcpy(out, c->d_order + c->groups[G_FX_HRTF].offset, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return GAS_OK;
}

int gas_bandwidth_probe(gas_ctx *c, uint64_t read_bytes, uint64_t write_bytes, uint32_t workgroups, uint32_t unroll, uint32_t iters, double *out_us) {
	if (!c || !out_us || iters == 0 || workgroups == 0 || read_bytes % 16 != 0 || write_bytes % 16 != 0 || read_bytes + write_bytes == 0) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	{ // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
		const int rcd = flush_deferred(c);
		if (rcd != GAS_OK) {
			return rcd;
		}
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	// the read arena is swept in rotation so that successive launches cannot be served by the 256 MiB Infinity Cache
	const size_t want_rd = read_bytes ? ((size_t)(320u << 20) / read_bytes + 2) * read_bytes : 16;
	if (want_rd > c->probe_rd_bytes) {
		GAS_HIP(c, c->mem.grow(c->d_probe_rd, c->probe_rd_bytes, want_rd));
		GAS_HIP(c, hipMemsetAsync(c->d_probe_rd, 0, want_rd, c->stream));
	}
	const size_t want_wr = write_bytes ? write_bytes : 16;
	GAS_HIP(c, c->mem.grow(c->d_probe_wr, c->probe_wr_bytes, want_wr));
	GAS_HIP(c, alloc_once(c, c->d_probe_sink, 256));
	Mem tmp; // destroys the two events on every way out
	hipEvent_t e0 = nullptr, e1 = nullptr;
	GAS_HIP(c, tmp.make_event(e0, hipEventDefault));
	GAS_HIP(c, tmp.make_event(e1, hipEventDefault));
	// marker calibration as in gas_profile_enable: an empty bracket, minimum of 16 tries
	double marker = 1e9;
	for (int i = 0; i < 16; i++) {
		GAS_HIP(c, hipEventRecord(e0, c->stream));
		GAS_HIP(c, hipEventRecord(e1, c->stream));
		GAS_HIP(c, hipEventSynchronize(e1));
		float ms = 0.0f;
		GAS_HIP(c, hipEventElapsedTime(&ms, e0, e1));
		marker = ms < marker ? ms : marker;
	}
	const size_t slices = read_bytes ? c->probe_rd_bytes / read_bytes : 1;
	size_t k = 0;
	auto launch = [&]() {
		const char *rd = static_cast<const char *>(c->d_probe_rd) + (k++ % slices) * read_bytes;
		return gas_launch_stream_probe(c->stream, rd, read_bytes, c->d_probe_wr, write_bytes, workgroups, unroll, c->d_probe_sink);
	};
	for (int i = 0; i < 8; i++) { // warm-up, back to back
		GAS_HIP(c, launch());
	}
	double sum_ms = 0.0;
	for (uint32_t i = 0; i < iters; i++) {
		GAS_HIP(c, launch()); // an unbracketed launch in front keeps the GPU busy, as the bench's callbacks do
		GAS_HIP(c, hipEventRecord(e0, c->stream));
		GAS_HIP(c, launch());
		GAS_HIP(c, hipEventRecord(e1, c->stream));
		GAS_HIP(c, hipEventSynchronize(e1));
		float ms = 0.0f;
		GAS_HIP(c, hipEventElapsedTime(&ms, e0, e1));
		sum_ms += ms > marker ? ms - marker : 0.0;
	}
	*out_us = sum_ms / iters * 1e3;
	return GAS_OK;
}

int gas_profile_read(gas_ctx *c, gas_profile *out, int reset) {
	if (!c || !out) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	{ // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first
		const int rcd = flush_deferred(c);
		if (rcd != GAS_OK) {
			return rcd;
		}
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	for (uint32_t i = 0; i + 1 < c->ev_used; i += 2) {
		float ms = 0.0f;
		GAS_HIP(c, hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
		c->prof_ms += ms > c->ev_overhead_ms ? ms - c->ev_overhead_ms : 0.0;
		c->prof_launches++;
	}
	c->ev_used = 0;
	std::memset(out, 0, sizeof(*out));
	out->launches = c->prof_launches;
	out->kernel_ms = c->prof_ms;
	out->bytes_per_launch = c->prof_bytes;
	out->callbacks_per_launch = c->prof_k;
	out->bytes_per_callback_formula = c->prof_k > 1 ? c->prof_bytes_formula : c->prof_bytes;
	if (c->prof_group >= 0) {
		std::string name = c->prof_multi ? "k_hrtf_multi" : (c->prof_uni ? "k_hrtf_uni" : k_group_kernel[c->prof_group]);
		if (c->prof_pipe && name.rfind("k_biquad_mix", 0) == 0) {
			name = "k_biquad_pipe" + name.substr(12);
		}
		std::strncpy(out->kernel_name, name.c_str(), sizeof(out->kernel_name) - 1);
	}
	if (reset) {
		c->prof_launches = 0;
		c->prof_ms = 0.0;
	}
	return GAS_OK;
}

// ---- bus convolvers (NEW; k_conv.hip) ---------------------------------------------------------------------------------

#define GAS_CONV_MAX_IR_TAPS (1u << 20)

static void conv_release(gas_ctx *c) {
	c->mem.drop(c->conv_pool.ring);
	c->mem.drop(c->conv_pool.prev);
	c->mem.drop(c->conv_pool.ypart);
	c->mem.drop(c->conv_w1024);
	c->mem.drop(c->conv_h_in);
	c->mem.drop(c->conv_h_out);
	c->mem.drop(c->conv_d_in);
	c->mem.drop(c->conv_d_out);
	c->conv_pool = gas_conv_pool{};
	c->conv_count = 0;
	c->conv_max_taps = 0;
	c->conv.clear();
	c->conv_free.clear();
	c->conv_irs.clear();
}

// The instance's ring and previous block become zeros in stream order: x[t] = 0 for every earlier t.
static hipError_t conv_zero(gas_ctx *c, uint32_t conv) {
	const size_t ring = (size_t)2 * c->conv_pool.K * GAS_CONV_BINS;
	const hipError_t e = hipMemsetAsync(c->conv_pool.ring + conv * ring, 0, ring * sizeof(float2), c->stream);
	return e != hipSuccess ? e : hipMemsetAsync(c->conv_pool.prev + (size_t)conv * 2 * 512, 0, 2 * 512 * sizeof(float), c->stream);
}

static bool conv_live(const gas_ctx *c, uint32_t conv) {
	return conv < c->conv_count && c->conv[conv].used;
}

static bool conv_ir_live(const gas_ctx *c, uint32_t ir) {
	return ir < c->conv_irs.size() && c->conv_irs[ir].H != nullptr;
}

// The fade in progress ends in state B: A's IR is no longer named, B's reference becomes the state's.
static void conv_fade_land(gas_ctx *c, gas_ctx::ConvInst &k) {
	c->conv_irs[k.ir].users--;
	k.ir = k.to.ir;
	k.dry = k.to.dry;
	k.wet = k.to.wet;
	k.fade_n = k.fade_pos = 0;
}

// gas_conv_set_ir, gas_conv_set_levels: a fade in progress ends at once in state B and a pending target is dropped.
static void conv_fade_end(gas_ctx *c, gas_ctx::ConvInst &k) {
	if (k.fade_n) {
		conv_fade_land(c, k);
	}
	if (k.pending_n) {
		c->conv_irs[k.pending.ir].users--;
		k.pending_n = 0;
	}
}

int gas_ctx_reserve_conv(gas_ctx *c, uint32_t convolvers, uint32_t max_ir_taps) {
	if (!c || convolvers > GAS_MAX_CONVOLVERS || max_ir_taps > GAS_CONV_MAX_IR_TAPS || (convolvers == 0) != (max_ir_taps == 0)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	for (const auto &k : c->conv) {
		if (k.used) {
			return GAS_ERR_INVALID_ARGUMENT;
		}
	}
	for (const auto &ir : c->conv_irs) {
		if (ir.H) {
			return GAS_ERR_INVALID_ARGUMENT;
		}
	}
	GAS_TRY(flush_deferred(c));
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	conv_release(c);
	if (convolvers == 0) {
		return GAS_OK;
	}
	const uint32_t F = c->cfg.frames;
	const uint32_t K = (max_ir_taps + F - 1) / F;
	const int rc = [&]() -> int {
		gas_conv_pool &p = c->conv_pool;
		p.K = K;
		p.max_chunks = gas_conv_max_chunks(K);
		GAS_HIP(c, c->mem.alloc(p.ring, (size_t)convolvers * 2 * K * GAS_CONV_BINS));
		GAS_HIP(c, c->mem.alloc(p.prev, (size_t)convolvers * 2 * 512));
		// two rows (ears) per named instance and two more per fading one: 96 rows of max_chunks spectra of 4 KiB,
		// 393 216 max_chunks bytes
		GAS_HIP(c, c->mem.alloc(p.ypart, (size_t)GAS_MAX_CONVOLVERS * 4 * p.max_chunks * GAS_CONV_BINS));
		GAS_HIP(c, c->mem.alloc(c->conv_w1024, 512));
		const size_t stage = (size_t)GAS_MAX_CONVOLVERS * F;
		GAS_HIP(c, c->mem.alloc(c->conv_h_in, stage, Mem::PINNED));
		GAS_HIP(c, c->mem.alloc(c->conv_h_out, stage, Mem::PINNED));
		GAS_HIP(c, c->mem.alloc(c->conv_d_in, stage));
		GAS_HIP(c, c->mem.alloc(c->conv_d_out, stage));
		float2 w[512];
		gas_make_w1024(w);
		GAS_HIP(c, hipMemcpyAsync(c->conv_w1024, w, sizeof(w), hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, hipStreamSynchronize(c->stream));
		p.w1024 = c->conv_w1024;
		return GAS_OK;
	}();
	if (rc != GAS_OK) {
		conv_release(c);
		return rc;
	}
	c->conv_count = convolvers;
	c->conv_max_taps = max_ir_taps;
	c->conv.assign(convolvers, gas_ctx::ConvInst{});
	c->conv_free.reserve(convolvers);
	for (uint32_t s = convolvers; s-- > 0;) {
		c->conv_free.push_back(s);
	}
	return GAS_OK;
}

// The common end of gas_conv_ir_load and gas_conv_ir_from_room: d_ir [channels][taps] is on the device, in the context's
// stream order.  Allocates the partition spectra, transforms, waits (the caller may free d_ir) and enters the IR in the
// table at the lowest free id.  A failure leaves no IR.
static int conv_ir_register(gas_ctx *c, const float *d_ir, uint32_t channels, uint32_t taps, uint32_t *out_ir) {
	const uint32_t F = c->cfg.frames;
	gas_ctx::ConvIr rec;
	rec.channels = channels;
	rec.taps = taps;
	rec.k_ir = (taps + F - 1) / F;
	GAS_HIP(c, c->mem.alloc(rec.H, (size_t)channels * rec.k_ir * GAS_CONV_BINS));
	hipError_t e = gas_launch_conv_ir(c->stream, d_ir, channels, taps, F, c->d_tw, c->conv_pool.w1024, rec.H);
	e = e != hipSuccess ? e : hipStreamSynchronize(c->stream);
	if (e != hipSuccess) {
		c->mem.drop(rec.H);
		GAS_HIP(c, e);
	}
	uint32_t id = 0;
	while (id < c->conv_irs.size() && c->conv_irs[id].H) {
		id++;
	}
	if (id == c->conv_irs.size()) {
		c->conv_irs.push_back(rec);
	} else {
		c->conv_irs[id] = rec;
	}
	*out_ir = id;
	return GAS_OK;
}

int gas_conv_ir_load(gas_ctx *c, const float *ir, uint32_t channels, uint32_t taps, uint32_t *out_ir) {
	if (!c || !ir || !out_ir || (channels != 1 && channels != 2 && channels != 4) || taps == 0) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (c->conv_count == 0) {
		return GAS_ERR_UNSUPPORTED_CHAIN;
	}
	if (taps > c->conv_max_taps) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	const size_t floats = (size_t)channels * taps;
	for (size_t i = 0; i < floats; i++) {
		if (!std::isfinite(ir[i])) {
			return GAS_ERR_INVALID_ARGUMENT;
		}
	}
	GAS_TRY(flush_deferred(c));
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	Mem tmp; // frees d_ir on every way out
	float *d_ir = nullptr;
	GAS_HIP(c, tmp.alloc(d_ir, floats));
	GAS_HIP(c, hipMemcpyAsync(d_ir, ir, floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
	return conv_ir_register(c, d_ir, channels, taps, out_ir);
}

// What gas_conv_ir_from_room and gas_conv_ir_from_room_hrtf refuse in a descriptor's plain fields; `ears`: ear_spacing too.
static bool room_ir_desc_ok(const gas_room_ir &d, bool ears) {
	const gas_room &R = d.room;
	bool ok = R.speed_of_sound > 0.0f && std::isfinite(R.speed_of_sound) && R.level >= 0.0f && std::isfinite(R.level); // gas_calc_early_reflections' test but for max_order
	for (int a = 0; a < 3; a++) {
		ok = ok && R.half_extent[a] > 0.0f && std::isfinite(R.half_extent[a]);
	}
	for (int w = 0; w < 6; w++) {
		ok = ok && R.reflectance[w] >= 0.0f && R.reflectance[w] <= 1.0f;
	}
	ok = ok && (d.max_order == 0 || d.min_order <= d.max_order);
	ok = ok && (!ears || (d.ear_spacing >= 0.0f && std::isfinite(d.ear_spacing)));
	for (int a = 0; a < 3; a++) {
		ok = ok && std::isfinite(R.origin[a]) && std::isfinite(d.source[a]) && std::isfinite(d.listener.origin[a]);
		for (int b = 0; b < 3; b++) {
			ok = ok && std::isfinite(R.basis[a][b]) && std::isfinite(d.listener.basis[a][b]);
		}
	}
	return ok;
}

// The HRIR set of gas_conv_ir_from_room_hrtf, as the caller passed it.
struct RoomIrSet {
	const float *hrir;
	uint32_t n_az, n_el, taps;
};

// The common body of the two box-room calls once everything is validated and the plan is made: tables, temporaries,
// the generator's launches inside the profile bracket, registration and read-back.  set == nullptr: k_room_ir with
// `channels` receivers; otherwise k_room_ir_hrtf, two ears.
static int conv_ir_from_plan(gas_ctx *c, const gas_room_ir &desc, const gas_room_ir_plan &plan, uint32_t channels, const RoomIrSet *set, float *out_taps, uint32_t *out_ir) {
	const uint32_t taps = plan.taps;
	std::vector<double> tables;
	try {
		tables.resize(gas_room_ir_table_doubles(plan));
	} catch (const std::bad_alloc &) {
		c->last_err = "gas_conv_ir_from_room: out of host memory for the reflectance tables";
		return GAS_ERR_DEVICE;
	}
	gas_room_ir_fill_tables(desc, plan, tables.data());
	if (out_ir) { // the pure generator leaves queued callbacks where they are: it touches nothing of theirs
		GAS_TRY(flush_deferred(c));
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	const size_t n = (size_t)channels * taps;
	Mem tmp; // frees the buffers on every way out
	double *d_tables = nullptr;
	long long *d_acc = nullptr;
	float *d_ir = nullptr, *d_hrir = nullptr;
	GAS_HIP(c, tmp.alloc(d_tables, tables.size()));
	GAS_HIP(c, tmp.alloc(d_acc, n));
	GAS_HIP(c, tmp.alloc(d_ir, n));
	GAS_HIP(c, hipMemcpy(d_tables, tables.data(), tables.size() * sizeof(double), hipMemcpyHostToDevice)); // complete on return
	if (set) {
		const size_t floats = (size_t)set->n_az * set->n_el * 2 * set->taps;
		GAS_HIP(c, tmp.alloc(d_hrir, floats));
		GAS_HIP(c, hipMemcpy(d_hrir, set->hrir, floats * sizeof(float), hipMemcpyHostToDevice));
	}
	const bool timed = c->profiling && c->ev_used + 2 <= c->ev.size(); // gas_profile_enable: the generator's launches count as a dominant launch
	if (timed) {
		GAS_HIP(c, hipEventRecord(c->ev[c->ev_used], c->stream));
	}
	if (set) {
		GAS_HIP(c, gas_launch_room_ir_hrtf(c->stream, plan, desc, d_tables, d_hrir, set->n_az, set->n_el, set->taps, d_acc, d_ir));
	} else {
		GAS_HIP(c, gas_launch_room_ir(c->stream, plan, d_tables, d_acc, d_ir));
	}
	if (timed) {
		GAS_HIP(c, hipEventRecord(c->ev[c->ev_used + 1], c->stream));
		c->ev_used += 2;
	}
	if (out_ir) { // waits for the stream
		uint32_t id = 0;
		GAS_TRY(conv_ir_register(c, d_ir, channels, taps, &id));
		if (out_taps) {
			const hipError_t e = hipMemcpy(out_taps, d_ir, n * sizeof(float), hipMemcpyDeviceToHost);
			if (e != hipSuccess) { // no IR and nothing reported: the caller's out_ir keeps its value
				c->mem.drop(c->conv_irs[id].H);
				c->conv_irs[id] = gas_ctx::ConvIr{};
				GAS_HIP(c, e);
			}
		}
		*out_ir = id;
		return GAS_OK;
	}
	GAS_HIP(c, hipStreamSynchronize(c->stream)); // before anything reaches out_taps: a failed kernel writes nothing there
	GAS_HIP(c, hipMemcpy(out_taps, d_ir, n * sizeof(float), hipMemcpyDeviceToHost));
	return GAS_OK;
}

int gas_conv_ir_from_room(gas_ctx *c, const gas_room_ir *desc, uint32_t channels, uint32_t taps, float *out_taps, uint32_t *out_ir) {
	if (!c || !desc || (!out_taps && !out_ir) || (channels != 1 && channels != 2) || taps == 0) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (out_ir && c->conv_count == 0) {
		return GAS_ERR_UNSUPPORTED_CHAIN;
	}
	if (taps > (out_ir ? c->conv_max_taps : (uint32_t)GAS_CONV_MAX_IR_TAPS)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	gas_room_ir_plan plan;
	if (!room_ir_desc_ok(*desc, true) || !gas_room_ir_make_plan(*desc, channels, taps, c->cfg.mix_rate, plan)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	return conv_ir_from_plan(c, *desc, plan, channels, nullptr, out_taps, out_ir);
}

int gas_conv_ir_from_room_hrtf(gas_ctx *c, const gas_room_ir *desc, const float *hrir, uint32_t n_az, uint32_t n_el, uint32_t hrir_taps, uint32_t taps, float *out_taps, uint32_t *out_ir) {
	if (!c || !desc || !hrir || (!out_taps && !out_ir) || taps == 0) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (n_az == 0 || n_el == 0 || (uint64_t)n_az * n_el > 65536u || hrir_taps == 0 || hrir_taps > GAS_HRTF_TAPS) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (out_ir && c->conv_count == 0) {
		return GAS_ERR_UNSUPPORTED_CHAIN;
	}
	if (taps > (out_ir ? c->conv_max_taps : (uint32_t)GAS_CONV_MAX_IR_TAPS)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	gas_room_ir_plan plan;
	if (!room_ir_desc_ok(*desc, false) || !gas_room_ir_make_plan(*desc, 1, taps, c->cfg.mix_rate, plan)) { // one receiver: ear_spacing is not read
		return GAS_ERR_INVALID_ARGUMENT;
	}
	const size_t floats = (size_t)n_az * n_el * 2 * hrir_taps;
	for (size_t i = 0; i < floats; i++) {
		if (!(std::fabs(hrir[i]) <= 4.0f)) { // not finite, or a tap could pass 4 v per image: the int64 sums' bound
			return GAS_ERR_INVALID_ARGUMENT;
		}
	}
	const RoomIrSet set{hrir, n_az, n_el, hrir_taps};
	return conv_ir_from_plan(c, *desc, plan, 2, &set, out_taps, out_ir);
}

int gas_conv_ir_free(gas_ctx *c, uint32_t ir) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (!conv_ir_live(c, ir)) {
		return GAS_ERR_BAD_SLOT;
	}
	if (c->conv_irs[ir].users != 0) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	GAS_TRY(flush_deferred(c));
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipStreamSynchronize(c->stream)); // calls still queued may read the spectra
	c->mem.drop(c->conv_irs[ir].H);
	c->conv_irs[ir] = gas_ctx::ConvIr{};
	return GAS_OK;
}

int gas_conv_ir_get_info(gas_ctx *c, uint32_t ir, uint32_t *out_channels, uint32_t *out_taps) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (!conv_ir_live(c, ir)) {
		return GAS_ERR_BAD_SLOT;
	}
	if (out_channels) {
		*out_channels = c->conv_irs[ir].channels;
	}
	if (out_taps) {
		*out_taps = c->conv_irs[ir].taps;
	}
	return GAS_OK;
}

int gas_conv_create(gas_ctx *c, uint32_t ir, uint32_t *out_conv) {
	if (!c || !out_conv) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (c->conv_count == 0) {
		return GAS_ERR_UNSUPPORTED_CHAIN;
	}
	if (!conv_ir_live(c, ir)) {
		return GAS_ERR_BAD_SLOT;
	}
	if (c->conv_free.empty()) {
		return GAS_ERR_OUT_OF_SLOTS;
	}
	const uint32_t id = c->conv_free.back();
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, conv_zero(c, id)); // zeroed when it changes hands
	c->conv_free.pop_back();
	gas_ctx::ConvInst &k = c->conv[id];
	k = gas_ctx::ConvInst{};
	k.used = true;
	k.ir = ir;
	k.pos = c->conv_pool.K - 1;
	c->conv_irs[ir].users++;
	*out_conv = id;
	return GAS_OK;
}

int gas_conv_destroy(gas_ctx *c, uint32_t conv) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (!conv_live(c, conv)) {
		return GAS_ERR_BAD_SLOT;
	}
	conv_fade_end(c, c->conv[conv]); // releases every IR the instance names
	c->conv_irs[c->conv[conv].ir].users--;
	c->conv[conv].used = false;
	c->conv_free.push_back(conv);
	return GAS_OK;
}

int gas_conv_reset(gas_ctx *c, uint32_t conv) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (!conv_live(c, conv)) {
		return GAS_ERR_BAD_SLOT;
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, conv_zero(c, conv));
	gas_ctx::ConvInst &k = c->conv[conv];
	k.pos = c->conv_pool.K - 1;
	if (k.fade_n) { // the fade ends in its final state: the pending target if there is one, else B
		conv_fade_land(c, k);
		if (k.pending_n) {
			k.to = k.pending;
			k.pending_n = 0;
			conv_fade_land(c, k);
		}
	}
	return GAS_OK;
}

int gas_conv_set_ir(gas_ctx *c, uint32_t conv, uint32_t ir) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (!conv_live(c, conv) || !conv_ir_live(c, ir)) {
		return GAS_ERR_BAD_SLOT;
	}
	conv_fade_end(c, c->conv[conv]);
	c->conv_irs[c->conv[conv].ir].users--;
	c->conv[conv].ir = ir;
	c->conv_irs[ir].users++;
	return GAS_OK;
}

int gas_conv_set_levels(gas_ctx *c, uint32_t conv, float dry, float wet) {
	if (!c || !std::isfinite(dry) || !std::isfinite(wet)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (!conv_live(c, conv)) {
		return GAS_ERR_BAD_SLOT;
	}
	conv_fade_end(c, c->conv[conv]);
	c->conv[conv].dry = dry;
	c->conv[conv].wet = wet;
	return GAS_OK;
}

int gas_conv_fade_to(gas_ctx *c, uint32_t conv, uint32_t ir, float dry, float wet, uint32_t fade_blocks) {
	if (!c || !std::isfinite(dry) || !std::isfinite(wet) || fade_blocks > GAS_CONV_MAX_FADE_BLOCKS) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (!conv_live(c, conv) || !conv_ir_live(c, ir)) {
		return GAS_ERR_BAD_SLOT;
	}
	if (fade_blocks == 0) { // nothing can refuse from here on
		gas_conv_set_ir(c, conv, ir);
		return gas_conv_set_levels(c, conv, dry, wet);
	}
	gas_ctx::ConvInst &k = c->conv[conv];
	gas_ctx::ConvTarget t;
	t.ir = ir;
	t.dry = dry;
	t.wet = wet;
	c->conv_irs[ir].users++;
	if (k.fade_n) { // waits for the fade in progress; the latest target wins
		if (k.pending_n) {
			c->conv_irs[k.pending.ir].users--;
		}
		k.pending = t;
		k.pending_n = fade_blocks;
	} else {
		k.to = t;
		k.fade_n = fade_blocks;
		k.fade_pos = 0;
	}
	return GAS_OK;
}

int gas_conv_fade_remaining(gas_ctx *c, uint32_t conv, uint32_t *out_blocks) {
	if (!c || !out_blocks) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (!conv_live(c, conv)) {
		return GAS_ERR_BAD_SLOT;
	}
	const gas_ctx::ConvInst &k = c->conv[conv];
	*out_blocks = k.fade_n - k.fade_pos + k.pending_n;
	return GAS_OK;
}

int gas_conv_process(gas_ctx *c, const uint32_t *convs, uint32_t n, const gas_audio_frame *in, gas_audio_frame *out, uint32_t frames, int mem) {
	if (!c || (mem != GAS_MEM_HOST && mem != GAS_MEM_DEVICE) || (n > 0 && (!convs || !in || !out))) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	const uint32_t F = c->cfg.frames;
	// a refused host-memory call leaves zeros in `out` ([n][frames] as the caller sized it, as far as that is legal)
	const size_t zero_bytes = out ? (size_t)(n < GAS_MAX_CONVOLVERS ? n : GAS_MAX_CONVOLVERS) * (frames < 512 ? frames : 512) * sizeof(gas_audio_frame) : 0;
	const auto fail = [&](int code) { return zero_bytes ? fail_out(code, mem, out, zero_bytes) : code; };
	if (n > GAS_MAX_CONVOLVERS) {
		return fail(GAS_ERR_INVALID_ARGUMENT);
	}
	if (frames != F) {
		return fail(GAS_ERR_FRAME_COUNT);
	}
	if (n == 0) {
		return GAS_OK;
	}
	uint32_t seen = 0;
	for (uint32_t i = 0; i < n; i++) {
		if (!conv_live(c, convs[i])) {
			return fail(GAS_ERR_BAD_SLOT);
		}
		if (seen & (1u << convs[i])) {
			return fail(GAS_ERR_INVALID_ARGUMENT); // an instance named twice
		}
		seen |= 1u << convs[i];
	}
	if (mem == GAS_MEM_DEVICE && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) != 0) {
		return fail(GAS_ERR_INVALID_ARGUMENT); // rows are read and written sixteen bytes at a time
	}
	{ // GAS_FLAG_BATCHED_LAUNCH: callbacks waiting for their batch run first (`in` may be one's out)
		const int rcd = flush_deferred(c);
		if (rcd != GAS_OK) {
			return fail(rcd);
		}
	}
	if (hipSetDevice(c->cfg.device) != hipSuccess) {
		return fail(GAS_ERR_NO_DEVICE);
	}
	if (mem == GAS_MEM_DEVICE) {
		const int rcj = join_outputs(c); // GAS_FLAG_PIPELINED_MIX: `in` may be an earlier callback's out, still a pending sum
		if (rcj != GAS_OK) {
			return rcj;
		}
	}
	const uint32_t K = c->conv_pool.K;
	gas_conv_call call{};
	for (uint32_t i = 0; i < n; i++) {
		const gas_ctx::ConvInst &k = c->conv[convs[i]];
		const gas_ctx::ConvIr &ir = c->conv_irs[k.ir];
		gas_conv_entry &e = call.e[i];
		e.H = ir.H;
		e.slot = convs[i];
		e.pos = k.pos + 1 == K ? 0 : k.pos + 1;
		e.k_ir = ir.k_ir;
		e.mode = gas_conv_mode(ir.channels);
		e.dry = k.dry;
		e.wet = k.wet;
		if (k.fade_n) { // call fade_pos of fade_n: frame i has s = (float)(fade_pos F + i) * (1.0f / (float)(fade_n F))
			const gas_ctx::ConvIr &irb = c->conv_irs[k.to.ir];
			e.HB = k.to.ir == k.ir ? nullptr : irb.H; // a level-only fade: the wet sum is computed once
			e.k_irB = irb.k_ir;
			e.modeB = gas_conv_mode(irb.channels);
			e.dryB = k.to.dry;
			e.wetB = k.to.wet;
			e.fade_t0 = k.fade_pos * F;
			e.fade_inv = 1.0f / (float)(k.fade_n * F);
		}
	}
	const size_t bytes = (size_t)n * F * sizeof(gas_audio_frame);
	const int rc = [&]() -> int {
		if (mem == GAS_MEM_DEVICE) {
			GAS_HIP(c, gas_launch_conv(c->stream, call, n, c->conv_pool, c->d_tw, in, out, F));
			return GAS_OK;
		}
		// host memory: the previous host-memory call returned after its copies, so the staging is free
		std::memcpy(c->conv_h_in, in, bytes);
		GAS_HIP(c, hipMemcpyAsync(c->conv_d_in, c->conv_h_in, bytes, hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, gas_launch_conv(c->stream, call, n, c->conv_pool, c->d_tw, c->conv_d_in, c->conv_d_out, F));
		GAS_HIP(c, hipMemcpyAsync(c->conv_h_out, c->conv_d_out, bytes, hipMemcpyDeviceToHost, c->stream));
		GAS_HIP(c, hipStreamSynchronize(c->stream));
		std::memcpy(out, c->conv_h_out, bytes);
		return GAS_OK;
	}();
	if (rc != GAS_OK) {
		return fail(rc);
	}
	for (uint32_t i = 0; i < n; i++) {
		gas_ctx::ConvInst &k = c->conv[convs[i]];
		k.pos = call.e[i].pos; // only the named instances' time advances, and only their fades
		if (k.fade_n && ++k.fade_pos == k.fade_n) { // that was the fade's last call: state B, A's IR may be freed
			conv_fade_land(c, k);
			if (k.pending_n) { // the pending fade starts at the next call, from B
				k.to = k.pending;
				k.fade_n = k.pending_n;
				k.pending_n = 0;
			}
		}
	}
	return GAS_OK;
}

} // extern "C"
