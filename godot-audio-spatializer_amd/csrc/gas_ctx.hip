// gas_ctx.hip -- the C ABI of include/gas_amd.h: context life cycle, device-resident playback-data slots, parameter
// publication, the grouping of a callback's slot list (build_groups) and the callback bodies that stand in for
// AudioSpatializerInstance::_mix_from_playback_list (audio_spatializer.cpp:326-471).
// Behind gas_ctx_priv.h: what a callback launches is gas_ctx_run.hip (run_groups), the effect families are
// gas_ctx_fx.hip, and the entries off the callback path live in gas_ctx_conv.hip (bus convolvers), gas_ctx_streams.hip
// (stream control, fed rows), gas_ctx_calc.hip (parameter generators) and gas_ctx_hrtf_profile.hip.
//
// There is NO CPU fallback: every entry needs a HIP device and fails with GAS_ERR_NO_DEVICE /
// GAS_ERR_DEVICE otherwise.
#include "gas_ctx_priv.h"

namespace gas_priv __attribute__((visibility("hidden"))) {

// The parameter flushes and feed_drop: entries in the other units call them too (gas_ctx_priv.h).

// Scatter a deferred device-side publish into the table (list unchanged since it was recorded).
int flush_pending_params(gas_ctx *c) {
	if (!c->pending_params) {
		return GAS_OK;
	}
	const gas_params *p = c->pending_params;
	c->pending_params = nullptr;
	GAS_HIP(c, gas_launch_scatter_params(c->stream, c->st.params, p, c->list.identity_rows ? c->list.d_slots : c->list.d_slots_rows, c->pending_n));
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

inline bool wants_peak(const gas_ctx *c, const SlotInfo &si) {
	return si.draining || !(c->cfg.flags & GAS_FLAG_PEAKS_DRAINING_ONLY);
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
		fx_slot_freed(c, s, si.chain_sig);
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
	list_invalidate(c);
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

// build_groups, step 1: may the list run?  Fills counts[] with its entries per launch group.  Writes nothing but the
// duplicate stamp and makes no HIP call: a rejected list leaves the cached one's arrays as they were.
int check_list(gas_ctx *c, const uint32_t *slots, uint32_t n, bool all_staged, uint32_t *counts) {
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
	return GAS_OK;
}

// build_groups, step 2: the counting sort.  Writes each group's offset and count, and h_idx: the slots, then each one's
// row in the caller's list, in group order (input order kept inside a group).  Returns the number of non-empty groups.
int sort_by_group(gas_ctx *c, const uint32_t *slots, uint32_t n, bool all_staged, const uint32_t *counts) {
	SlotList &l = c->list;
	uint32_t off = 0, cursor[G_COUNT];
	int nonempty = 0;
	for (int gt = 0; gt < G_COUNT; gt++) {
		l.groups[gt].offset = off;
		l.groups[gt].count = counts[gt];
		cursor[gt] = off;
		off += counts[gt];
		nonempty += counts[gt] > 0;
	}
	uint32_t *hs = l.h_idx, *hr = l.h_idx + c->cfg.max_sources;
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t p = cursor[launch_group(c, c->slots[slots[i]], all_staged)]++;
		hs[p] = slots[i];
		hr[p] = i;
	}
	return nonempty;
}

// build_groups, step 3: runs of equal chains inside the staged group (stable: input order kept within a run), as
// chain_ranges.  h_idx is final behind it, so what is read off the final order is settled here too: which groups are
// one slot range, and whether the sorted order is the caller's (`nonempty`: sort_by_group's count).
void chain_runs(gas_ctx *c, int nonempty) {
	SlotList &l = c->list;
	uint32_t *hs = l.h_idx, *hr = l.h_idx + c->cfg.max_sources;
	l.chain_ranges.clear();
	if (l.groups[G_FX_GENERIC].count) {
		const Group &gg = l.groups[G_FX_GENERIC];
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
			if (l.chain_ranges.empty() || l.chain_ranges.back().sig != sig) {
				ChainRange r;
				r.sig = sig;
				r.offset = k;
				l.chain_ranges.push_back(r);
			}
			l.chain_ranges.back().count++;
		}
	}
	for (int gt = 0; gt < G_COUNT; gt++) {
		Group &gr = l.groups[gt];
		gr.contiguous = gr.count > 0;
		gr.slot_base = gr.count ? hs[gr.offset] : 0;
		for (uint32_t k = 1; k < gr.count && gr.contiguous; k++) {
			gr.contiguous = hs[gr.offset + k] == gr.slot_base + k;
		}
	}
	l.identity_rows = nonempty <= 1 && l.chain_ranges.size() <= 1;
}

// build_groups, step 4: which entries report their exact peak -- the plain-[HRTF] group's summary and bits (k_hrtf_uni),
// then each staged run's.  A table goes to the device only where some entries do and some do not: at most two copies.
int peak_bits(gas_ctx *c) {
	SlotList &l = c->list;
	const uint32_t *hs = l.h_idx;
	l.uni_peak_all = l.uni_peak_any = false;
	if (uni_ok(c) && l.groups[G_FX_HRTF].count > 0) {
		const Group &gh = l.groups[G_FX_HRTF];
		const uint32_t words = (gh.count + 31) / 32;
		std::memset(l.h_peak_bits, 0, (size_t)words * sizeof(uint32_t));
		uint32_t n_peak = 0;
		for (uint32_t k = 0; k < gh.count; k++) {
			if (wants_peak(c, c->slots[hs[gh.offset + k]])) {
				l.h_peak_bits[k >> 5] |= 1u << (k & 31);
				n_peak++;
			}
		}
		l.uni_peak_any = n_peak > 0;
		l.uni_peak_all = n_peak == gh.count;
		if (l.uni_peak_any && !l.uni_peak_all) {
			GAS_HIP(c, hipMemcpyAsync(l.d_peak_bits, l.h_peak_bits, (size_t)words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		}
	}
	// staged chains whose last stage is k_hrtf_uni: the same rule (an HRTF source that is not draining reports +inf)
	if (uni_ok(c) && (c->cfg.flags & GAS_FLAG_PEAKS_DRAINING_ONLY) != 0 && l.groups[G_FX_GENERIC].count > 0) {
		const Group &gg = l.groups[G_FX_GENERIC];
		const uint32_t half = (c->cfg.max_sources + 31) / 32, words = (gg.count + 31) / 32;
		uint32_t *bits = l.h_peak_bits + half;
		std::memset(bits, 0, (size_t)words * sizeof(uint32_t));
		bool partial = false;
		for (ChainRange &r : l.chain_ranges) {
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
			GAS_HIP(c, hipMemcpyAsync(l.d_peak_bits + half, bits, (size_t)words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		}
	}
	return GAS_OK;
}

// build_groups, step 5: the sorted slots -- with the rows and the caller's order where the order is not the caller's
// -- to the device, and the commit: the only step that sets `valid` and `n` and starts a generation.
int upload_commit(gas_ctx *c, const uint32_t *slots, uint32_t n) {
	SlotList &l = c->list;
	const uint32_t *hs = l.h_idx, *hr = l.h_idx + c->cfg.max_sources;
	if (n > 0) {
		GAS_HIP(c, hipMemcpyAsync(l.d_slots, hs, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		if (!l.identity_rows) {
			GAS_HIP(c, hipMemcpyAsync(l.d_rows, hr, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
			GAS_HIP(c, hipMemcpyAsync(l.d_slots_rows, slots, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		}
		GAS_HIP(c, hipStreamSynchronize(c->stream)); // h_idx is reused by the next list
	}
	l.valid = true;
	l.n = n;
	l.gen++;
	return GAS_OK;
}

// The callback's slot list becomes c->list: validated and counting-sorted by launch group.  The cached list is given
// up first, so a list that is rejected, or whose upload fails, leaves none to reuse.  all_staged
// (gas_process_block_buses over effect kinds): every chain runs staged (rows out), the rows are mixed per bus.
int build_groups(gas_ctx *c, const uint32_t *slots, uint32_t n, bool all_staged) {
	list_invalidate(c);
	uint32_t counts[G_COUNT] = { 0 };
	GAS_TRY(check_list(c, slots, n, all_staged, counts));
	const int nonempty = sort_by_group(c, slots, n, all_staged, counts);
	chain_runs(c, nonempty);
	GAS_TRY(peak_bits(c));
	return upload_commit(c, slots, n);
}

int needs_hrtf(const gas_ctx *c) {
	bool any = c->list.groups[G_FX_HRTF].count > 0 || c->list.groups[G_FX_ER_HRTF].count > 0 || c->list.groups[G_FX_HRTF_PK].count > 0 || c->list.groups[G_FX_ER_HRTF_PK].count > 0;
	for (const ChainRange &r : c->list.chain_ranges) {
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
		GAS_TRY(fx_create(c)); // the effect families that need no reservation for their settings
		GAS_HIP(c, c->mem.alloc(c->d_upload, N));
		GAS_HIP(c, c->mem.alloc(c->d_upload_slots, N));
		GAS_HIP(c, c->mem.alloc(c->list.d_slots, N));
		GAS_HIP(c, c->mem.alloc(c->list.d_rows, N));
		GAS_HIP(c, c->mem.alloc(c->list.d_slots_rows, N));
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
		GAS_HIP(c, c->mem.alloc(c->list.h_idx, 2 * N, Mem::PINNED));
		GAS_HIP(c, c->mem.alloc(c->list.h_peak_bits, 2 * ((N + 31) / 32), Mem::PINNED));
		GAS_HIP(c, c->mem.alloc(c->list.d_peak_bits, 2 * ((N + 31) / 32)));
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
	std::lock_guard<std::mutex> alloc_lk(c->alloc_mu); // any thread (instantiate_playback_data runs on the physics thread, audio_spatializer.cpp:69)
	GAS_TRY(fx_room(c, effects, n_effects)); // no pool reserved (gas_ctx_reserve_fx_*), or a pool without room
	if (c->free_list.empty()) { // all or nothing: nothing has been taken yet
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
	fx_slot_new(c, s, effects, n_effects, sig);
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
		list_invalidate(c); // launch groups change: the next callback must pass its slot list again
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
	fx_slot_reset(c, slot); // its pool entries: zeroed by the next flush, before the next block
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
		if (!list_serves(c, n)) {
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

// What every callback body begins with: the caller's frame count is the context's, and the context's device is current.
int callback_begin(const gas_ctx *c, uint32_t frames) {
	if (frames != c->cfg.frames) {
		return GAS_ERR_FRAME_COUNT;
	}
	return hipSetDevice(c->cfg.device) == hipSuccess ? GAS_OK : GAS_ERR_NO_DEVICE;
}

// GAS_FLAG_BATCHED_LAUNCH: may the callbacks that wait for their batch go on waiting while this one joins them?  Only
// a device-memory callback over the very list, grouping and parameters they were recorded with.
bool deferred_still_valid(const gas_ctx *c, const uint32_t *slots, uint32_t n, int mem, bool host_dirty) {
	return mem == GAS_MEM_DEVICE && !slots && n == c->deferred_n && c->pending_free.empty() && c->list.gen == c->deferred_groups_gen && !host_dirty;
}

// May a bus callback run n entries without being handed the list?  On the cached list, where the last bus callback ran
// it in a form whose grouping is the ordinary one, and no free waits to regroup it.
bool bus_list_reusable(const gas_ctx *c, uint32_t n) {
	return list_serves(c, n) && c->list.bus_form != BUS_FORM_NONE && c->pending_free.empty();
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
			host_dirty = !c->dirty_list.empty() || fx_basic_dirty(c) || !c->blend_dirty_list.empty();
		}
		if (!deferred_still_valid(c, slots, n, mem, host_dirty)) {
			GAS_TRY(flush_deferred(c));
		}
	}
	// Device-published rows are scattered with the mapping they were published for -- c->list's device arrays, which
	// outlive an invalidation -- so in front of anything below that may rebuild them.
	if (c->pending_params && (slots || n == 0 || !list_serves(c, n) || !c->pending_free.empty())) {
		GAS_TRY(flush_pending_params(c));
	}
	apply_pending_frees(c);
	if (slots || n == 0) { // an empty callback needs no list
		GAS_TRY(build_groups(c, slots, n, false));
	} else if (!list_serves(c, n)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (needs_hrtf(c)) {
		return GAS_ERR_NO_HRTF;
	}
	const uint64_t pgen = c->params_gen.load(); // read before the snapshot: a publish racing with it re-sorts next time
	GAS_TRY(flush_params(c)); // one snapshot per callback (audio_spatializer.cpp:328)
	if (c->order_groups_gen != c->list.gen || c->order_params_gen != pgen) {
		std::memset(c->order_ok, 0, sizeof(c->order_ok));
		c->order_groups_gen = c->list.gen;
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
			only_hrtf = only_hrtf && (gt == G_FX_HRTF || gt == G_FX_HRTF_PK || gt == G_FX_ER_HRTF || gt == G_FX_ER_HRTF_PK || c->list.groups[gt].count == 0);
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
		c->deferred_groups_gen = c->list.gen;
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
	const BusForm cached_form = c->list.bus_form; // read in front of apply_pending_frees: frees adopted only now take the list away
	GAS_TRY(flush_pending_params(c));
	apply_pending_frees(c);
	// Two forms: every source GAS_KIND_3D_MIX (the mix-channel buses of AudioSpatializer3D, fused in the biquad
	// kernels), or every source an effect chain (run staged: per-source rows, then mixed per bus) on a one-pair context.
	const bool reuse = n > 0 && !slots; // bus_list_reusable held: the list ran as 3D mix or as fused [HRTF]
	const BusList form = reuse ? (cached_form == BUS_FORM_3D_MIX ? BUS_LIST_3D_MIX : BUS_LIST_PLAIN_HRTF) : bus_list_form(c, slots, n);
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
		GAS_TRY(build_groups(c, slots, n, staged));
		if (staged) {
			list_invalidate(c); // the staged grouping is this call's only: a later list reuse must regroup
		}
	}
	if (c->list.valid) { // the form a later bus callback may run it in again
		c->list.bus_form = fused_hrtf ? BUS_FORM_FUSED_HRTF : (form == BUS_LIST_3D_MIX ? BUS_FORM_3D_MIX : BUS_FORM_NONE);
	}
	for (int gt = 0; gt < G_COUNT; gt++) {
		if (gt != (staged ? G_FX_GENERIC : (fused_hrtf ? G_FX_HRTF : G_3D_MIX)) && c->list.groups[gt].count > 0) {
			list_invalidate(c);
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
		ga.rows = c->list.identity_rows ? nullptr : c->list.d_rows;
		ga.slots = c->list.d_slots;
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
	if (n > 0 && !slots && !bus_list_reusable(c, n)) {
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
			&& (list_serves(c, n) || (buses && s.bus_staged)) // the staged bus form regroups on every call and leaves no cached groups behind: its list stays "the same" without them
			&& s.last_buses == buses
			&& s.groups_gen == c->list.gen
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
		list_invalidate(c);
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
		const bool reuse = same_list && n > 0 && bus_list_reusable(c, n);
		rc = process_block_buses(c, rows, reuse ? nullptr : slots, n, F, d_out, n_buses, d_pk, GAS_MEM_DEVICE);
		c->streams.bus_staged = rc == GAS_OK && n > 0 && c->list.bus_form == BUS_FORM_NONE; // it ran staged: nothing cached to compare with next time
	} else {
		rc = process_block(c, rows, same_list ? nullptr : slots, n, F, d_out, d_pk, GAS_MEM_DEVICE);
	}
	c->streams.groups_gen = rc == GAS_OK ? c->list.gen : UINT64_MAX;
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
