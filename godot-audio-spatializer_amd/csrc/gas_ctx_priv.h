// gas_ctx_priv.h -- what the units of the C ABI (gas_ctx.hip and gas_ctx_*.hip) share: the context, its types, the
// error macros, and what the units call of each other: the launch plan (gas_ctx_run.hip), the effect families
// (gas_ctx_fx.hip) and the few helpers of gas_ctx.hip that entries in other units call.  Declarations and inlines only.
#pragma once
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
#include "gas_switches.h"

// Hidden: the library is built without -fvisibility, and none of these names belongs in its dynamic symbol table.
namespace gas_priv __attribute__((visibility("hidden"))) {

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

inline const char *const k_group_kernel[G_COUNT] = {
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

// The form a gas_process_block_buses ran the list in, where a later bus callback may run it again without being handed
// the list.  NONE: no bus callback ran it, or it ran staged -- a grouping of that call alone.
enum BusForm { BUS_FORM_NONE = 0, BUS_FORM_3D_MIX, BUS_FORM_FUSED_HRTF };

// The slot list a callback leaves behind for the next one (slots == NULL, the stream entries' "same list again", the
// batched launch, the direction order), as c->list: what build_groups writes, and build_groups alone -- its last step
// commits `valid`, `n` and a new `gen`; list_invalidate takes `valid` away; bus_body notes the form it ran.
// !valid: no caller may reuse the list (list_serves).  Its device arrays stay where they are all the same: they are the
// mapping of device-published rows not scattered yet (pending_params, recorded while the list was valid), so
// flush_pending_params runs before the next build_groups overwrites them -- every callback body flushes, or has seen
// that nothing is pending, in front of its rebuild.
// Whoever caches something derived from the list keeps the `gen` it was derived from (deferred_groups_gen,
// order_groups_gen, streams.groups_gen).
struct SlotList {
	uint32_t n = 0;
	bool valid = false;
	uint64_t gen = 0; // one per committed rebuild
	BusForm bus_form = BUS_FORM_NONE; // reset by every rebuild and every invalidation: it needs no generation of its own
	bool identity_rows = true; // the sorted order is the caller's row order
	Group groups[G_COUNT];
	std::vector<ChainRange> chain_ranges; // sub-runs of groups[G_FX_GENERIC]
	// plain [HRTF] group (k_hrtf_uni): which entries need their exact peak
	bool uni_peak_all = false, uni_peak_any = false;
	// host and device mirrors (the context's Mem owns them)
	uint32_t *h_idx = nullptr; // pinned [2 * max_sources]: slots then rows, sorted by group
	uint32_t *d_slots = nullptr, *d_rows = nullptr; // sorted by launch group
	uint32_t *d_slots_rows = nullptr; // the caller's list in row order (device-side parameter publication)
	uint32_t *h_peak_bits = nullptr, *d_peak_bits = nullptr; // two halves of (max_sources + 31) / 32 words: bit k = entry k of the plain-[HRTF] group / of the staged group
};

constexpr uint32_t PROFILE_EVENTS = 4096;

// The effect families, in the order their uploads are flushed; gas_ctx_fx.hip's table describes them.  The
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
struct ConvState {
	uint32_t count = 0, max_taps = 0; // the reservation; 0: none
	gas_conv_pool pool{};
	float2 *w1024 = nullptr;
	std::vector<ConvInst> inst;
	std::vector<uint32_t> free; // pop_back hands out 0, 1, 2, ...
	std::vector<ConvIr> irs;
	gas_audio_frame *h_in = nullptr, *h_out = nullptr; // pinned [GAS_MAX_CONVOLVERS][frames], host-memory calls
	gas_audio_frame *d_in = nullptr, *d_out = nullptr;
};

// gas_calc_spatialization staging (physics thread)
struct CalcState {
	std::mutex mu;
	SlotStamp stamp; // duplicate detection in a call's slot list (under mu)
	gas_spatializer3d_config *d_cfgs = nullptr;
	gas_listener *d_listeners = nullptr;
	uint32_t *d_slots = nullptr, *d_cfgidx = nullptr;
	gas_source_pose *d_poses = nullptr;
	gas_params *d_out = nullptr;
	gas_area_send *d_areas = nullptr; // gas_calc_spatialization_areas staging (host-memory calls)
	float *d_lap = nullptr;
	gas_audio_frame *d_reverb = nullptr;
	gas_room *d_rooms = nullptr; // gas_calc_early_reflections: its rooms (everything else it stages lies in the buffers above)
};

// gas_bandwidth_probe: read arena (larger than the Infinity Cache, swept in rotation) and write target
struct ProbeState {
	void *d_rd = nullptr, *d_wr = nullptr;
	size_t rd_bytes = 0, wr_bytes = 0;
	float *d_sink = nullptr;
};

// device-resident streams and playback cursors: the streams, each playback's cursor, and what the
// stream callbacks (gas_ctx.hip) keep of their last list.  Audio-thread state.
struct StreamInfo {
	void *d_pcm = nullptr;
	uint64_t frames = 0;
	uint32_t format = 0, channels = 0;
	bool resampled = false; // its playbacks are [ENGINE] AudioStreamPlaybackResampled (gas_stream_set_resampled)
	uint32_t loop_mode = 0; // NEW gas_stream_set_loop: its playbacks repeat [loop_begin, loop_end)
	uint64_t loop_begin = 0, loop_end = 0;
};
struct StreamRow { // compact mirror of the cached list's cursors: the per-callback host loop touches only this
	uint64_t remaining = 0;
	uint32_t has_frames = 0, draining_marked = 0;
	uint32_t resampled = 0, inc = 65536; // resampled playbacks: 16.16 step of this callback (from the host-published pitch_scale)
	uint64_t fp_pos = 0, end_fp = 0; // ... and the engine's mix_offset / the stream's end, 16.16
	uint32_t looped = 0; // gas_stream_set_loop: never ends; a plain playback counts `pos` up instead of `remaining` down
	uint64_t pos = 0;
};
struct StreamListTraits { // of the cached list, rebuilt with it (stream_list_adopt)
	bool all_hrtf = false; // every playback a plain [HRTF] chain
	bool any_resampled = false;
	bool any_looped = false;
	bool any_adpcm = false; // a GAS_PCM_IMA_ADPCM playback: rows first, k_sample_adpcm behind k_sample_sources
	bool any_qoa = false; // a GAS_PCM_QOA playback: rows first, k_sample_qoa behind k_sample_sources
};
struct StreamState {
	std::vector<StreamInfo> info; // by stream id; d_pcm null: a free id
	gas_cursor *d_cursors = nullptr; // [max_sources]
	std::vector<gas_cursor> h_cursors; // host mirror of the cursor arithmetic (deterministic, no read-back)
	uint32_t *d_slots = nullptr; // callback slot list in row order
	uint32_t *d_inc = nullptr, *h_inc = nullptr; // [max_sources] 16.16 step per row (resampled playbacks)
	std::vector<uint32_t> slots_host; // what d_slots / the cached launch groups currently hold
	std::vector<StreamRow> rows;
	StreamListTraits list;
	uint64_t groups_gen = UINT64_MAX; // list.gen the stream path's cached list corresponds to
	bool last_fused = false; // the last stream callback that got as far as its launches sampled inside the HRTF kernel (gas_stream_last_fused)
	bool last_buses = false; // the cached stream list was validated by gas_process_block_streams_buses (its checks differ from the mix entry's)
	bool bus_staged = false; // ... and ran the staged bus form, which regroups on every call (c->list never serves it)
	bool params_touched = false; // a parameter publish may have changed pitch_scale: re-validate
};

// gas_source_feed_rows: window rows of playbacks that are not bound to a stream, pending for the next stream callback.
// d_table is the feed table the kernels read (gas_internal.h, GAS_FEED_*): [max_sources] words in the callback's row
// order, then two halves of max_sources rows: the rows of every call since the last callback, appended as they came
// (feed_place).
struct FeedState {
	uint8_t *d_table = nullptr;
	size_t used = 0; // end of the rows taken, as an offset into d_table (0: emptied)
	uint32_t side = 0; // the half of the table that rows are appended in
	std::vector<uint32_t> moved; // feed_place: (slot, new word) of the rows it moved to the other half
	uint8_t *h_rows = nullptr; // pinned staging of one GAS_MEM_HOST call
	size_t h_cap = 0;
	hipEvent_t ev = nullptr; // the last upload out of h_rows
	std::vector<uint32_t> word; // [max_sources] by slot: GAS_FEED_NONE, or where and in which format its pending row lies
	std::vector<uint32_t> slots; // the slots with a pending row
	std::vector<uint32_t> entry, entry_dev; // per list entry: this callback's words, and the words the table's header holds (empty: none written)
	uint32_t *h_entry = nullptr; // [max_sources] pinned: what the header upload reads
	hipEvent_t entry_ev = nullptr; // ... and the last upload out of it
};

// gas_profile_enable: event pairs around launches, and what the last timed launch was.
struct ProfState {
	bool on = false;
	std::vector<hipEvent_t> ev;
	uint32_t ev_used = 0;
	double ev_overhead_ms = 0.0; // marker/dispatch overhead of an event pair around one launch (calibrated)
	uint32_t every = 1, tick = 0; // bracket every Nth launch that asks
	uint64_t launches = 0;
	double ms = 0.0;
	uint64_t bytes = 0, bytes_formula = 0;
	uint32_t k = 1;
	int group = -1;
	bool uni = false, multi = false, pipe = false; // the timed launch was k_hrtf_uni / k_hrtf_multi / k_biquad_pipe
	// The bracket of one launch: `timed = room() [&& due()]`, begin() in front of the launch, end() behind it.
	bool room() const { // profiling, and two events are free
		return on && ev_used + 2 <= ev.size();
	}
	bool due() { // this asker's turn; call it only where room() holds, it counts the askers
		return (tick++ % every) == 0;
	}
	hipError_t begin(hipStream_t s) const {
		return hipEventRecord(ev[ev_used], s);
	}
	hipError_t end(hipStream_t s) {
		const hipError_t e = hipEventRecord(ev[ev_used + 1], s);
		ev_used += e == hipSuccess ? 2 : 0;
		return e;
	}
};

} // namespace gas_priv
using namespace gas_priv; // the units name these types and helpers as gas_ctx.hip always did

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
	uint32_t partial_planes = 1; // planes of d_partials (1 ordered, 2 pipelined, 2 x max batch depth batched)
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

	SlotList list; // the cached slot list
	// parameter rows published from device memory for it (row order), not yet in the table
	const gas_params *pending_params = nullptr;
	uint32_t pending_n = 0;
	std::atomic<uint64_t> params_gen{ 1 }; // bumped by every call that can change a source's HRIR direction
	uint32_t *d_order = nullptr; // [max_sources] direction order of the frequency-domain HRTF groups (k_dir_order)
	uint64_t order_groups_gen = UINT64_MAX, order_params_gen = 0; // what d_order was built from
	bool order_ok[G_COUNT] = {}; // d_order holds this group's order
	bool last_uni_ordered = false; // the last k_hrtf_uni launch ran in k_xcd_order's order
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

	StreamState streams;
	float *d_fade_env = nullptr; // [64]
	FeedState feed;

	CalcState calc;

	// several output buses: slot-indexed routes, host mirror + device table, own partial planes
	std::vector<gas_bus_route> h_routes; // guarded by params_mu
	bool routes_dirty = false;
	gas_bus_route *h_routes_pinned = nullptr, *d_routes = nullptr;
	float *d_bus_partials = nullptr;
	size_t bus_partial_floats = 0;
	gas_audio_frame *d_bus_out = nullptr; // [GAS_MAX_BUSES][C][F] staging for host-memory calls

	ConvState conv;
	ProbeState probe;

	ProfState prof;
	gas_switches sw; // the environment's run-time switches, filled once by gas_ctx_create (gas_switches.h)
	bool uni_er_enabled = true; // sw.uni_er_mode != 0, and no GAS_FLAG_ER_TAP_FADE (gas_ctx_create)

	std::string last_err;
};

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

namespace gas_priv __attribute__((visibility("hidden"))) {

// The slot names a playback of this context.
inline bool live(const gas_ctx *c, uint32_t slot) {
	return slot < c->cfg.max_sources && c->slots[slot].used;
}

// The one place that says "no list": launch groups changed, a list was rejected, or the grouping was one call's only.
inline void list_invalidate(gas_ctx *c) {
	c->list.valid = false;
	c->list.bus_form = BUS_FORM_NONE;
}

// May a caller that names no list (slots == NULL, "the same list again") run n entries on the cached one?
inline bool list_serves(const gas_ctx *c, uint32_t n) {
	return c->list.valid && c->list.n == n;
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

// Marks row s of a slot-indexed host mirror for the next flush; params_mu held.
inline void mark_dirty(std::vector<uint8_t> &flag, std::vector<uint32_t> &list, uint32_t s) {
	if (!flag[s]) {
		flag[s] = 1;
		list.push_back(s);
	}
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

// gas_ctx_run.hip: what a callback launches
uint32_t chain_signature(const int32_t *fx, uint32_t n_fx);
bool chain_has(uint32_t sig, int kind);
RunArgs own_list(const gas_ctx *c, const RowSource &src, uint32_t n, gas_audio_frame *out, float *peaks);
gas_group_args own_hrtf_group(const gas_ctx *c, const gas_audio_frame *src, uint32_t n, float *peaks);
gas_biquad_launch biquad_launch(const gas_ctx *c, int mode, const gas_group_args &g, float *partials, uint32_t p_offset);
gas_hrtf_uni_launch plain_uni_launch(const gas_ctx *c, const gas_group_args &g, const RowSource &src, float *partials, uint32_t p_offset);
int run_groups(gas_ctx *c, const RunArgs &a);
bool batchable(const gas_ctx *c, uint32_t n, bool fused);
int flush_deferred(gas_ctx *c);
int join_outputs(gas_ctx *c);

// gas_ctx_fx.hip: the effect families.  Nothing else names their table or a member of FxFamily.
int family_of(int kind);
hipError_t fx_launch(const gas_ctx *c, int kind, const gas_group_args &in, uint32_t chain_pos, gas_audio_frame *rows_out);
int fx_create(gas_ctx *c); // gas_ctx_create: the resident families' tables, staging and mirrors
int fx_room(const gas_ctx *c, const int32_t *effects, uint32_t n_effects); // gas_source_alloc, alloc_mu held: GAS_OK, GAS_ERR_UNSUPPORTED_CHAIN or GAS_ERR_OUT_OF_SLOTS
void fx_slot_new(gas_ctx *c, uint32_t s, const int32_t *effects, uint32_t n_effects, uint32_t sig); // ... then the new slot's entries and defaults
void fx_slot_freed(gas_ctx *c, uint32_t s, uint32_t sig); // apply_pending_frees, alloc_mu held
void fx_slot_reset(gas_ctx *c, uint32_t s); // gas_source_reset: takes alloc_mu, then params_mu
int fx_flush(gas_ctx *c, int f);
bool fx_basic_dirty(const gas_ctx *c); // params_mu held

// gas_ctx.hip's, called by entries in the other units
int fail_out(int code, int mem, gas_audio_frame *out, size_t out_bytes);
void feed_drop(gas_ctx *c, uint32_t slot);
void stream_rows_sync_back(gas_ctx *c);
int flush_pending_params(gas_ctx *c);
int flush_hrtf_blend(gas_ctx *c);
int flush_param_rows(gas_ctx *c);

} // namespace gas_priv
