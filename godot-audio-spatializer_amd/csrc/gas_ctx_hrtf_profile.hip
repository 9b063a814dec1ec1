// gas_ctx_hrtf_profile.hip -- HRIR set loading (gas_hrtf_load*) and the measuring entries: gas_profile_enable / _read,
// gas_bandwidth_probe, gas_ctx_read_hrtf_order.
#include "gas_ctx_priv.h"

extern "C" {

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
	if (on && c->prof.ev.empty()) {
		std::vector<hipEvent_t> ev(PROFILE_EVENTS, nullptr);
		for (hipEvent_t &e : ev) {
			GAS_HIP(c, c->mem.make_event(e, hipEventDefault)); // a failure leaves c->prof.ev empty and what exists to the owner
		}
		c->prof.ev = std::move(ev);
	}
	if (on) {
		// An event pair around a launch reads the launch's span on the GPU timeline plus the cost of the second
		// marker.  Only the marker is calibrated away (an empty bracket, minimum of 16 tries): the dispatch ramp of
		// the kernel itself stays in, exactly as rocprofv3's kernel trace counts it (an empty kernel reads 3-4 us
		// there), so the two figures of one run agree and neither flatters the kernel.
		GAS_HIP(c, hipStreamSynchronize(c->stream));
		double best = 1e9;
		for (int i = 0; i < 16; i++) {
			GAS_HIP(c, hipEventRecord(c->prof.ev[0], c->stream));
			GAS_HIP(c, hipEventRecord(c->prof.ev[1], c->stream));
			GAS_HIP(c, hipEventSynchronize(c->prof.ev[1]));
			float ms = 0.0f;
			GAS_HIP(c, hipEventElapsedTime(&ms, c->prof.ev[0], c->prof.ev[1]));
			best = ms < best ? ms : best;
		}
		c->prof.ev_overhead_ms = best;
	}
	c->prof.on = on != 0;
	c->prof.every = on > 1 ? (uint32_t)on : 1; // on = N > 1: bracket every Nth callback only (the markers cost throughput)
	c->prof.tick = 0;
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
	for (uint32_t i = 0; i + 1 < c->prof.ev_used; i += 2) {
		float ms = 0.0f;
		GAS_HIP(c, hipEventElapsedTime(&ms, c->prof.ev[i], c->prof.ev[i + 1]));
		c->prof.ms += ms > c->prof.ev_overhead_ms ? ms - c->prof.ev_overhead_ms : 0.0;
		c->prof.launches++;
	}
	c->prof.ev_used = 0;
	std::memset(out, 0, sizeof(*out));
	out->launches = c->prof.launches;
	out->kernel_ms = c->prof.ms;
	out->bytes_per_launch = c->prof.bytes;
	out->callbacks_per_launch = c->prof.k;
	out->bytes_per_callback_formula = c->prof.k > 1 ? c->prof.bytes_formula : c->prof.bytes;
	if (c->prof.group >= 0) {
		std::string name = c->prof.multi ? "k_hrtf_multi" : (c->prof.uni ? "k_hrtf_uni" : k_group_kernel[c->prof.group]);
		if (c->prof.pipe && name.rfind("k_biquad_mix", 0) == 0) {
			name = "k_biquad_pipe" + name.substr(12);
		}
		std::strncpy(out->kernel_name, name.c_str(), sizeof(out->kernel_name) - 1);
	}
	if (reset) {
		c->prof.launches = 0;
		c->prof.ms = 0.0;
	}
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
	if (want_rd > c->probe.rd_bytes) {
		GAS_HIP(c, c->mem.grow(c->probe.d_rd, c->probe.rd_bytes, want_rd));
		GAS_HIP(c, hipMemsetAsync(c->probe.d_rd, 0, want_rd, c->stream));
	}
	const size_t want_wr = write_bytes ? write_bytes : 16;
	GAS_HIP(c, c->mem.grow(c->probe.d_wr, c->probe.wr_bytes, want_wr));
	GAS_HIP(c, alloc_once(c, c->probe.d_sink, 256));
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
	const size_t slices = read_bytes ? c->probe.rd_bytes / read_bytes : 1;
	size_t k = 0;
	auto launch = [&]() {
		const char *rd = static_cast<const char *>(c->probe.d_rd) + (k++ % slices) * read_bytes;
		return gas_launch_stream_probe(c->stream, rd, read_bytes, c->probe.d_wr, write_bytes, workgroups, unroll, c->probe.d_sink);
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
	if (!c->d_order || !c->order_ok[G_FX_HRTF] || !c->last_uni_ordered || n > c->list.groups[G_FX_HRTF].count) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipStreamSynchronize(c->stream));
	GAS_HIP(c, hipMemcpy(out, c->d_order + c->list.groups[G_FX_HRTF].offset, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return GAS_OK;
}

} // extern "C"
