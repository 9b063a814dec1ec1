// gas_ctx_streams.hip -- device-resident streams off the callback path: the gas_stream_* control entries,
// gas_source_bind_stream and gas_source_feed_rows.  The stream callbacks themselves are gas_ctx.hip's.
#include "gas_ctx_priv.h"

namespace {

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
	if (!c->feed.d_table) {
		if (alloc_once(c, c->feed.h_entry, c->cfg.max_sources, Mem::PINNED) != hipSuccess) {
			return GAS_ERR_OUT_OF_MEMORY;
		}
		if (!c->feed.entry_ev) {
			GAS_HIP(c, c->mem.make_event(c->feed.entry_ev, hipEventDisableTiming));
		}
		if (c->mem.alloc(c->feed.d_table, hdr + 2 * half) != hipSuccess) {
			return GAS_ERR_OUT_OF_MEMORY;
		}
		c->feed.used = 0;
	}
	if (c->feed.used < hdr) { // emptied by a callback: start over
		c->feed.used = hdr;
		c->feed.side = 0;
	}
	c->feed.moved.clear();
	switched = false;
	if (c->feed.used + bytes <= hdr + (c->feed.side + 1) * half) {
		at = c->feed.used;
		return GAS_OK;
	}
	switched = true;
	const uint32_t F = c->cfg.frames;
	size_t off = hdr + (1 - c->feed.side) * half;
	for (uint32_t s : c->feed.slots) {
		if (c->stamp.has(s)) {
			continue; // this call replaces it
		}
		const uint32_t w = c->feed.word[s];
		const size_t rb = gas_feed_row_bytes(w, F);
		GAS_HIP(c, hipMemcpyAsync(c->feed.d_table + off, c->feed.d_table + gas_feed_offset(w), rb, hipMemcpyDeviceToDevice, c->stream));
		c->feed.moved.push_back(s);
		c->feed.moved.push_back(gas_feed_word(off, (w & 2u) ? GAS_PCM_F32 : GAS_PCM_S16, (w & 1u) + 1u));
		off += rb;
	}
	at = off;
	return GAS_OK;
}

} // namespace

extern "C" {

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
	StreamInfo si;
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
	for (size_t i = 0; i < c->streams.info.size(); i++) {
		if (!c->streams.info[i].d_pcm) {
			c->streams.info[i] = si;
			*out_stream = (uint32_t)i;
			return GAS_OK;
		}
	}
	c->streams.info.push_back(si);
	*out_stream = (uint32_t)c->streams.info.size() - 1;
	return GAS_OK;
}

int gas_stream_set_resampled(gas_ctx *c, uint32_t stream, int on) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (stream >= c->streams.info.size() || !c->streams.info[stream].d_pcm) {
		return GAS_ERR_BAD_SLOT;
	}
	for (const gas_cursor &cur : c->streams.h_cursors) {
		if (cur.pcm == c->streams.info[stream].d_pcm) {
			return GAS_ERR_INVALID_ARGUMENT; // the playback class is chosen before playbacks are bound
		}
	}
	c->streams.info[stream].resampled = on != 0;
	return GAS_OK;
}

int gas_stream_set_loop(gas_ctx *c, uint32_t stream, int mode, uint64_t loop_begin, uint64_t loop_end) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (stream >= c->streams.info.size() || !c->streams.info[stream].d_pcm) {
		return GAS_ERR_BAD_SLOT;
	}
	StreamInfo &si = c->streams.info[stream];
	for (const gas_cursor &cur : c->streams.h_cursors) {
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
	if (stream >= c->streams.info.size() || !c->streams.info[stream].d_pcm) {
		return GAS_ERR_BAD_SLOT;
	}
	if (out_mode) {
		*out_mode = (int)c->streams.info[stream].loop_mode;
	}
	if (out_begin) {
		*out_begin = c->streams.info[stream].loop_begin;
	}
	if (out_end) {
		*out_end = c->streams.info[stream].loop_end;
	}
	return GAS_OK;
}

int gas_stream_destroy(gas_ctx *c, uint32_t stream) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (stream >= c->streams.info.size() || !c->streams.info[stream].d_pcm) {
		return GAS_ERR_BAD_SLOT;
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	for (gas_cursor &cur : c->streams.h_cursors) {
		if (cur.pcm == c->streams.info[stream].d_pcm) {
			return GAS_ERR_INVALID_ARGUMENT; // still bound to a playback
		}
	}
	c->mem.drop(c->streams.info[stream].d_pcm);
	c->streams.info[stream] = StreamInfo{};
	return GAS_OK;
}

int gas_stream_get_info(gas_ctx *c, uint32_t stream, uint64_t *out_frames, uint32_t *out_channels, int *out_format) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (stream >= c->streams.info.size() || !c->streams.info[stream].d_pcm) {
		return GAS_ERR_BAD_SLOT;
	}
	if (out_frames) {
		*out_frames = c->streams.info[stream].frames;
	}
	if (out_channels) {
		*out_channels = c->streams.info[stream].channels;
	}
	if (out_format) {
		*out_format = (int)c->streams.info[stream].format;
	}
	return GAS_OK;
}

int gas_source_bind_stream(gas_ctx *c, uint32_t slot, uint32_t stream, uint64_t start_frame) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (slot >= c->cfg.max_sources || !c->slots[slot].used || stream >= c->streams.info.size() || !c->streams.info[stream].d_pcm) {
		return GAS_ERR_BAD_SLOT;
	}
	stream_rows_sync_back(c);
	c->streams.groups_gen = UINT64_MAX;
	feed_drop(c, slot); // gas_source_feed_rows: the stream supplies the windows from here on
	const StreamInfo &si = c->streams.info[stream];
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
	c->streams.h_cursors[slot] = cur;
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipMemcpyAsync(c->streams.d_cursors + slot, &c->streams.h_cursors[slot], sizeof(gas_cursor), hipMemcpyHostToDevice, c->stream));
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	if (c->slots[slot].draining) {
		c->slots[slot].draining = 0;
		list_invalidate(c);
	}
	return GAS_OK;
}

int gas_stream_positions(gas_ctx *c, uint32_t n, uint64_t *out_frames) {
	if (!c || (n > 0 && !out_frames)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (n != c->streams.slots_host.size()) {
		return GAS_ERR_INVALID_ARGUMENT; // not the list of the last stream callback (gas_process_block_streams or gas_process_block_streams_buses)
	}
	// The compact row mirror holds the positions while the list is cached; a block boundary that applied deferred
	// frees has folded it back into the per-slot cursors (stream_rows_sync_back) and emptied it.
	const bool rows_live = c->streams.rows.size() == n;
	for (uint32_t i = 0; i < n; i++) {
		const gas_cursor &cur = c->streams.h_cursors[c->streams.slots_host[i]];
		if (!cur.pcm) {
			out_frames[i] = 0;
		} else if (rows_live) {
			const StreamRow &r = c->streams.rows[i];
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
		if (c->streams.h_cursors[slots[i]].pcm) {
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
	if (mem == GAS_MEM_HOST && bytes > c->feed.h_cap) { // grows to the largest call: not in the steady state
		if (c->feed.ev) {
			GAS_HIP(c, hipEventSynchronize(c->feed.ev));
		} else {
			GAS_HIP(c, c->mem.make_event(c->feed.ev, hipEventDisableTiming));
		}
		if (c->mem.grow(c->feed.h_rows, c->feed.h_cap, bytes, 1, Mem::PINNED) != hipSuccess) {
			return GAS_ERR_OUT_OF_MEMORY;
		}
	}
	size_t at = 0;
	bool switched = false;
	const int rcp = feed_place(c, bytes, at, switched);
	if (rcp != GAS_OK) {
		return rcp;
	}
	uint8_t *dst = c->feed.d_table + at;
	const int rcc = [&]() -> int {
		if (mem == GAS_MEM_DEVICE) {
			const int rcj = join_outputs(c); // GAS_FLAG_PIPELINED_MIX: `rows` may be an earlier callback's out, still a pending sum
			if (rcj != GAS_OK) {
				return rcj;
			}
			GAS_HIP(c, hipMemcpyAsync(dst, rows, bytes, hipMemcpyDeviceToDevice, c->stream));
			return GAS_OK;
		}
		GAS_HIP(c, hipEventSynchronize(c->feed.ev)); // the previous upload has left the staging: a wait only while it is still queued
		std::memcpy(c->feed.h_rows, rows, bytes);
		GAS_HIP(c, hipMemcpyAsync(dst, c->feed.h_rows, bytes, hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, hipEventRecord(c->feed.ev, c->stream));
		return GAS_OK;
	}();
	if (rcc != GAS_OK) {
		return rcc; // nothing committed: every pending row is still where its word says
	}
	if (switched) {
		c->feed.side = 1 - c->feed.side;
		for (size_t k = 0; k + 1 < c->feed.moved.size(); k += 2) {
			c->feed.word[c->feed.moved[k]] = c->feed.moved[k + 1];
		}
	}
	for (uint32_t i = 0; i < n; i++) {
		if (c->feed.word[slots[i]] == GAS_FEED_NONE) {
			c->feed.slots.push_back(slots[i]);
		} // else: replaces the row fed before; its bytes lie idle until the table is emptied
		c->feed.word[slots[i]] = gas_feed_word(at + (size_t)i * row_bytes, format, channels);
	}
	c->feed.used = at + bytes;
	return GAS_OK;
}

} // extern "C"
