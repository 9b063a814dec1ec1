// gas_ctx_run.hip -- what a callback launches: the launch plan of one callback over already-grouped entries
// (run_groups), the batched form of several (run_hrtf_batch), and the pending sums of GAS_FLAG_PIPELINED_MIX.  The
// callback bodies in gas_ctx.hip fill a RunArgs and call run_groups; the names they share with this unit are declared
// in gas_ctx_priv.h and defined in the second half of this file, everything in the first half is file-local.
#include "gas_ctx_priv.h"

namespace {

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
	return c->list.uni_peak_any && !c->list.uni_peak_all ? c->list.d_peak_bits : nullptr;
}

// What run_groups decides before it enqueues anything (plan_run).
struct RunPlan {
	bool uni_hrtf = false, staged_uni = false, uni_er = false; // the launch forms plan_partials counted the rows of
	uint32_t pcount[G_COUNT] = {}; // partial rows per group
	uint32_t p_total = 0, p_mix = 0; // ... of all groups, and of the mix_channel group (which come first)
	bool pipelined = false; // this callback's sum is left to the next one (GAS_FLAG_PIPELINED_MIX)
	int carrier_gt = -1; // the frequency-domain group whose launch takes the previous callback's sum along
	bool carrier = false; // ... and it can
	int dom = -1; // the dominant group: its launch is the one the profiler times
};

// What run_groups' loop over the groups shares with the launch families below.
struct GroupRun {
	const RunPlan &plan;
	float *parts = nullptr; // this callback's plane of d_partials
	uint32_t p_off = 0; // its rows taken by the groups in front of the current one
	gas_deferred_reduce job; // the previous callback's sum (GAS_FLAG_PIPELINED_MIX), until a launch takes it along
	// The job if fd_gt's launch is the carrier (`bytes`: what summing it adds to the launch's traffic), else none.
	gas_deferred_reduce take(int fd_gt, uint64_t &bytes) {
		if (fd_gt != plan.carrier_gt) {
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
	if (gt == G_FX_HRTF && gp.count == 0 && run.plan.uni_hrtf) {
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
	if (fd_gt == G_FX_ER_HRTF && run.plan.uni_er) {
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
		pp += range_partials(r, run.plan.staged_uni);
		gas_group_args in = ga;
		in.n = r.count;
		in.slots = d_slots + off;
		in.rows = d_rows ? d_rows + off : nullptr;
		in.src = d_rows ? d_src : d_src + (size_t)off * F; // identity rows: the run's first row is entry `off`
		in.peaks = d_rows ? a.peaks : a.peaks + (size_t)off * 2;
		const uint32_t *peak_rows = in.rows;
		const bool last_is_uni = range_ends_in_uni(r, run.plan.staged_uni);
		const bool own = a.groups == c->list.groups; // the context's own list: GAS_FLAG_PEAKS_DRAINING_ONLY's bits exist
		const int k0 = r.sig & 0xff;
		// a last stage that is k_hrtf_uni: exact peaks for every source of the chain, or (GAS_FLAG_PEAKS_DRAINING_ONLY,
		// the context's own list) for the draining ones
		gas_hrtf_uni_launch lu{ hrtf_common(c) };
		lu.peak_bits = own && r.peak_any && !r.peak_all ? c->list.d_peak_bits + (c->cfg.max_sources + 31) / 32 : nullptr;
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
			GAS_HIP(c, gas_launch_rows_accumulate_buses(c->stream, fin, F, a.buses->routes, a.buses->n_buses, run.plan.p_total, run.parts, pp_r));
		} else {
			GAS_HIP(c, gas_launch_rows_accumulate(c->stream, fin, F, run.parts, pp_r));
		}
	}
	return GAS_OK;
}

// run_groups, step 1: the plan.  A function of (c, a): no HIP call, nothing written to the context.
RunPlan plan_run(const gas_ctx *c, const RunArgs &a) {
	const uint32_t F = c->cfg.frames;
	const Group *const groups = a.groups;
	RunPlan p;
	p.uni_hrtf = groups == c->list.groups && uni_ok(c);
	p.staged_uni = uni_ok(c) && a.buses == nullptr && gas_hrtf_uni_waves() == 8; // staged chains ending in the HRTF: last stage = k_hrtf_uni
	// [ER, HRTF] through k_hrtf_uni<ER> (22.5 -> see profiles/r03_notes.md): the exact-peak group's entries follow the
	// frequency-domain group's in the callback's list, so one launch covers both
	const bool uni_er_pays = c->sw.uni_er_mode == 2 || groups[G_FX_ER_HRTF_PK].count * 4 <= groups[G_FX_ER_HRTF].count + groups[G_FX_ER_HRTF_PK].count;
	p.uni_er = uni_ok(c) && a.buses == nullptr && gas_hrtf_uni_waves() == 8 && c->uni_er_enabled && uni_er_pays && (groups[G_FX_ER_HRTF].count == 0 || groups[G_FX_ER_HRTF_PK].count == 0 || groups[G_FX_ER_HRTF].offset + groups[G_FX_ER_HRTF].count == groups[G_FX_ER_HRTF_PK].offset);
	plan_partials(groups, *a.ranges, p.pcount, p.uni_hrtf, p.staged_uni, p.uni_er);
	for (int gt = 0; gt < G_COUNT; gt++) {
		p.p_total += p.pcount[gt];
		if (gt == G_3D_MIX) {
			p.p_mix = p.p_total;
		}
	}
	// GAS_FLAG_PIPELINED_MIX: only callbacks that are one channel pair wide and carry an HRTF launch defer their sum
	p.pipelined = a.pipelined && c->pipelined_mix && a.channel_count == 1 && c->cfg.channel_count == 1;
	// A launch can carry the pending sum when it is the plain [HRTF] kernel (register budget), covers every output
	// column with a workgroup and the pending callback left at most 256 partial rows (k_hrtf_ols: job_issue).
	// The plain [HRTF] launch takes it when there is one, else the [ER, HRTF] launch.
	if (!a.src.fused() && (c->cfg.flags & (GAS_FLAG_HRTF_CROSSFADE | GAS_FLAG_HRTF_INTERPOLATE)) == 0) {
		for (int gt : { (int)G_FX_HRTF, (int)G_FX_ER_HRTF }) {
			if (p.carrier_gt < 0 && groups[gt].count + groups[gt + 1].count > 0) {
				p.carrier_gt = gt;
			}
		}
	}
	if (p.carrier_gt >= 0) {
		// the oldest pending sum is the one a single launch carries; with none pending the launch counts as fitting (the
		// join in settle_pending then has nothing to do either way)
		const bool fits = c->pending.empty() || c->pending.front().p_total <= 256;
		p.carrier = (p.pcount[p.carrier_gt] + p.pcount[p.carrier_gt + 1]) * GAS_HRTF_JOB_WAVES >= F * 2 / 4 && fits;
	}
	for (int gt = 0; gt < G_COUNT; gt++) {
		if (groups[gt].count > 0 && (p.dom < 0 || groups[gt].count > groups[p.dom].count)) {
			p.dom = gt;
		}
	}
	if ((p.dom == G_FX_HRTF_PK || p.dom == G_FX_ER_HRTF_PK) && groups[p.dom - 1].count > 0) {
		p.dom = p.dom - 1; // one launch covers both
	}
	return p;
}

// run_groups, step 2: the pending sums and the partial planes.  Behind it at most one sum is left, as run.job for the
// carrier's launch; run.parts is this callback's plane, `parity` its number; the peaks are zeroed where a launch
// accumulates them.
int settle_pending(gas_ctx *c, const RunArgs &a, const RunPlan &plan, GroupRun &run, int &parity) {
	const uint32_t p_rows = plan.p_total > 0 ? plan.p_total : 1;
	if (c->pending.size() > 1) { // left by a batched launch: a single launch carries one sum only, the oldest
		const std::vector<gas_ctx::PendingMix> more(c->pending.begin() + 1, c->pending.end());
		c->pending.resize(1);
		for (const gas_ctx::PendingMix &pm : more) {
			GAS_TRY(reduce_now(c, pm));
		}
	}
	if (!plan.pipelined || !plan.carrier || p_rows > c->partial_rows) {
		GAS_TRY(join_outputs(c)); // nobody to carry the pending sum (or the partials are about to move): do it now
	}
	GAS_TRY(ensure_partials(c, p_rows * (a.buses ? a.buses->n_buses : 1u))); // buses: p_total rows per bus, bus after bus
	parity = plan.pipelined ? free_plane(c, {}) : 0;
	run.parts = partials_plane(c, parity);
	if (!c->pending.empty()) { // handed to the carrier's launch
		run.job = carried_job(c, c->pending.front());
		c->pending.clear();
	}
	// only the mix_channel launch over several channel pairs accumulates peaks (atomicMax over the pairs, from zero);
	// every other launch -- a single pair included -- stores them, so the zeroing pass (a 4 us dispatch) is skipped
	if (a.groups[G_3D_MIX].count + a.groups[G_3D_PROCESS].count > 0 && a.channel_count > 1 && a.force_mode != GAS_MODE_PROCESS_FRAMES) {
		GAS_HIP(c, hipMemsetAsync(a.peaks, 0, (size_t)a.n_total * 2 * sizeof(float), c->stream));
	}
	return GAS_OK;
}

// run_groups, step 3: the launch of group gt (not empty).  `mode`: the gas_biquad_mode of a 3D group; `carried`: bytes
// of the previous callback's partial mixes summed inside this launch (GAS_FLAG_PIPELINED_MIX).
int launch_one_group(gas_ctx *c, const RunArgs &a, int gt, int mode, GroupRun &run, uint64_t &carried) {
	const Group &gr = a.groups[gt];
	gas_group_args ga;
	ga.src = a.src.rows; // nullptr when fused: only plain-[HRTF] launches run then, and they sample
	ga.rows = a.rows ? a.rows + gr.offset : nullptr;
	ga.slots = a.slots + gr.offset;
	ga.slot_base = 0;
	ga.n = gr.count;
	ga.peaks = a.peaks;
	switch (gt) {
		case G_3D_MIX:
		case G_3D_PROCESS: {
			gas_biquad_launch lb = biquad_launch(c, mode, ga, run.parts, run.p_off);
			if (mode == GAS_MODE_MIX_CHANNEL) {
				lb.channel_begin = a.channel_begin;
				lb.channel_count = a.channel_count;
			}
			GAS_HIP(c, gas_launch_biquad_mix(lb));
		} break;
		case G_FX_COPY:
			GAS_HIP(c, gas_launch_biquad_mix(biquad_launch(c, GAS_MODE_COPY, ga, run.parts, run.p_off)));
			break;
		case G_FX_SHELF:
			GAS_HIP(c, gas_launch_biquad_mix(biquad_launch(c, GAS_MODE_FX_HIGHSHELF, ga, run.parts, run.p_off)));
			break;
		case G_FX_ER:
			GAS_HIP(c, gas_launch_er_only(c->stream, ga, c->st, c->cfg.frames, c->cfg.er_ring_frames, run.parts, run.p_off, c->partial_rows, nullptr, er_fade_on(c)));
			break;
		case G_FX_HRTF_PK:
		case G_FX_ER_HRTF_PK:
			if (a.groups[gt - 1].count > 0) {
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
	return GAS_OK;
}

// run_groups, step 4: what the profiler keeps of the timed launch, group gt's (`mode`, `carried`: as in launch_one_group).
void record_timed(gas_ctx *c, const RunArgs &a, const RunPlan &plan, int gt, int mode, uint64_t carried) {
	const Group *const groups = a.groups;
	c->prof.bytes = group_bytes(c, gt, groups[gt].count) + carried;
	c->prof.k = 1;
	if ((gt == G_FX_HRTF || gt == G_FX_ER_HRTF) && groups[gt + 1].count > 0) {
		// the exact-peak sources ride in the same launch: add their per-source bytes (table/mix terms counted once)
		c->prof.bytes += group_bytes(c, gt + 1, groups[gt + 1].count) - group_bytes(c, gt + 1, 0);
	}
	c->prof.group = gt;
	c->prof.uni = (gt == G_FX_HRTF && plan.uni_hrtf && groups[G_FX_HRTF_PK].count == 0) || ((gt == G_FX_ER_HRTF || gt == G_FX_ER_HRTF_PK) && plan.uni_er);
	c->prof.multi = false;
	c->prof.pipe = (gt == G_3D_MIX || gt == G_3D_PROCESS || gt == G_FX_SHELF) && gas_biquad_uses_pipe(c->sw.biquad_pipe, gt == G_FX_SHELF ? GAS_MODE_FX_HIGHSHELF : mode, groups[gt].count, gt == G_3D_MIX ? a.channel_count : 1, c->cfg.frames, false);
}

// run_groups, step 5: the final sums -- left pending for the next callback's launch (pipelined), or launched now:
// channel pair 0 sums every group's partials; pairs > 0 only the mix_channel group's (which come first).
int final_sums(gas_ctx *c, const RunArgs &a, const RunPlan &plan, const GroupRun &run, int parity) {
	const uint32_t F = c->cfg.frames;
	if (run.job.partials) { // no launch took the pending sum along (cannot happen with hrtf_launch set; kept for safety)
		GAS_HIP(c, gas_launch_mix_reduce(c->stream, run.job.partials, run.job.p_count, c->partial_rows, 1, F, reinterpret_cast<gas_audio_frame *>(run.job.out)));
	}
	if (plan.pipelined) { // summed by the next callback's HRTF launch, gas_ctx_join_outputs or the next ordered call
		gas_ctx::PendingMix pm;
		pm.parity = parity;
		pm.p_total = plan.p_total;
		pm.out = a.out;
		c->pending.push_back(pm);
		c->pipe_tick++;
		return GAS_OK;
	}
	if (a.buses) { // out[b][F]: bus b's rows are [b * p_total, (b + 1) * p_total)
		GAS_HIP(c, gas_launch_mix_reduce(c->stream, run.parts, plan.p_total, plan.p_total > 0 ? plan.p_total : 1, a.buses->n_buses, F, a.out));
		return GAS_OK;
	}
	GAS_HIP(c, gas_launch_mix_reduce(c->stream, run.parts, plan.p_total, c->partial_rows, 1, F, a.out));
	if (a.channel_count > 1) {
		GAS_HIP(c, gas_launch_mix_reduce(c->stream, run.parts + (size_t)c->partial_rows * F * 2, plan.p_mix, c->partial_rows, a.channel_count - 1, F, a.out + F));
	}
	return GAS_OK;
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
	GAS_HIP(c, gas_launch_hrtf_multi(c->stream, ga, mb, plain_peak_bits(c), c->list.uni_peak_all, c->st, c->tab, c->d_tw, F, c->hist_len, c->d_partials));
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

} // namespace

namespace gas_priv __attribute__((visibility("hidden"))) {

// Effect kinds by chain position, 8 bits each, first effect in the low byte.  The digits keep their order, so sorting by
// signature orders chains of the kinds below 16 exactly as the earlier 4-bit digits did.
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

// Sums every pending callback now, on the context's stream.
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

// A callback over the context's own cached list.
RunArgs own_list(const gas_ctx *c, const RowSource &src, uint32_t n, gas_audio_frame *out, float *peaks) {
	RunArgs a;
	a.src = src;
	a.slots = c->list.d_slots;
	a.rows = c->list.identity_rows ? nullptr : c->list.d_rows;
	a.groups = c->list.groups;
	a.ranges = &c->list.chain_ranges;
	a.n_total = n;
	a.out = out;
	a.peaks = peaks;
	return a;
}

// The plain-[HRTF] group of the context's own list, for a launch that covers exactly it.
gas_group_args own_hrtf_group(const gas_ctx *c, const gas_audio_frame *src, uint32_t n, float *peaks) {
	const Group &gr = c->list.groups[G_FX_HRTF];
	gas_group_args ga;
	ga.src = src;
	ga.rows = c->list.identity_rows ? nullptr : c->list.d_rows + gr.offset;
	ga.slots = gr.contiguous ? nullptr : c->list.d_slots + gr.offset; // a contiguous slot range needs no list on the device
	ga.slot_base = gr.contiguous ? gr.slot_base : 0;
	ga.n = n;
	ga.peaks = peaks;
	return ga;
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

// k_hrtf_uni over the plain-[HRTF] group `g` of the context's own list.
gas_hrtf_uni_launch plain_uni_launch(const gas_ctx *c, const gas_group_args &g, const RowSource &src, float *partials, uint32_t p_offset) {
	gas_hrtf_uni_launch lu{ hrtf_common(c) };
	lu.g = g;
	lu.peak_bits = plain_peak_bits(c);
	lu.peak_all = c->list.uni_peak_all;
	lu.partials = partials;
	lu.p_offset = p_offset;
	lu.cursors = src.cursors;
	lu.feed = src.feed;
	return lu;
}

// Device work of one callback over already-grouped entries: plan, settle what earlier callbacks left pending, one
// launch per group in group order (the profiler's bracket around the dominant one), the final sums.
int run_groups(gas_ctx *c, const RunArgs &a) {
	const RunPlan plan = plan_run(c, a);
	GroupRun run{ plan };
	int parity = 0;
	GAS_TRY(settle_pending(c, a, plan, run, parity));
	for (int gt = 0; gt < G_COUNT; gt++) {
		if (a.groups[gt].count == 0) {
			continue;
		}
		const int mode = a.force_mode >= 0 ? a.force_mode : (gt == G_3D_MIX ? GAS_MODE_MIX_CHANNEL : GAS_MODE_PROCESS_FRAMES); // read for the 3D groups only
		const bool timed = gt == plan.dom && c->prof.room() && c->prof.due();
		if (timed) {
			GAS_HIP(c, c->prof.begin(c->stream));
		}
		uint64_t carried = 0;
		GAS_TRY(launch_one_group(c, a, gt, mode, run, carried));
		if (timed) {
			GAS_HIP(c, c->prof.end(c->stream));
			record_timed(c, a, plan, gt, mode, carried);
		}
		run.p_off += plan.pcount[gt];
	}
	return final_sums(c, a, plan, run, parity);
}

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
		if (gt != G_FX_HRTF && c->list.groups[gt].count != 0) {
			return false;
		}
	}
	const uint32_t wgs = gas_hrtf_uni_partials(n);
	// every wave of the launch has a source; every output column of a carried sum finds a job wave
	return c->list.groups[G_FX_HRTF].count == n && n >= wgs * gas_hrtf_uni_waves() && wgs * GAS_HRTF_JOB_WAVES >= c->cfg.frames * 2 / 4 && wgs <= 256;
}

} // namespace gas_priv
