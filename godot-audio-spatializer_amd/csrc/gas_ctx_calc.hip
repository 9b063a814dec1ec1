// gas_ctx_calc.hip -- the parameter generators of include/gas_amd.h: gas_calc_spatialization, its areas form and
// gas_calc_early_reflections (k_calc_spatialization.hip, k_calc_er.hip).
#include "gas_ctx_priv.h"

extern "C" {

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
	std::lock_guard<std::mutex> lk(c->calc.mu);
	c->calc.stamp.next();
	for (uint32_t i = 0; i < n; i++) {
		if (c->calc.stamp.seen(slots[i])) {
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
	GAS_HIP(c, hipMemcpyAsync(c->calc.d_cfgs, cfgs, sizeof(gas_spatializer3d_config) * n_cfgs, hipMemcpyHostToDevice, c->stream));
	if (n_listeners) {
		GAS_HIP(c, hipMemcpyAsync(c->calc.d_listeners, listeners, sizeof(gas_listener) * n_listeners, hipMemcpyHostToDevice, c->stream));
	}
	GAS_HIP(c, hipMemcpyAsync(c->calc.d_slots, slots, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
	if (cfg_index) {
		GAS_HIP(c, hipMemcpyAsync(c->calc.d_cfgidx, cfg_index, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
	}
	const gas_source_pose *d_poses = poses;
	gas_params *d_out = out_params;
	if (mem == GAS_MEM_HOST) {
		GAS_HIP(c, alloc_once(c, c->calc.d_poses, c->cfg.max_sources));
		GAS_HIP(c, hipMemcpyAsync(c->calc.d_poses, poses, sizeof(gas_source_pose) * n, hipMemcpyHostToDevice, c->stream));
		d_poses = c->calc.d_poses;
		if (out_params) {
			GAS_HIP(c, alloc_once(c, c->calc.d_out, c->cfg.max_sources));
			d_out = c->calc.d_out;
		}
	}
	const gas_area_send *d_areas = areas;
	const float *d_lap = listener_area_pos;
	gas_audio_frame *d_reverb = out_reverb;
	if (mem == GAS_MEM_HOST && (areas || out_reverb)) { // staged like the poses; sized for the worst case once
		GAS_HIP(c, alloc_once(c, c->calc.d_areas, c->cfg.max_sources));
		GAS_HIP(c, alloc_once(c, c->calc.d_lap, (size_t)3 * GAS_MAX_LISTENERS * c->cfg.max_sources));
		GAS_HIP(c, alloc_once(c, c->calc.d_reverb, (size_t)4 * c->cfg.max_sources));
		if (areas) {
			GAS_HIP(c, hipMemcpyAsync(c->calc.d_areas, areas, sizeof(gas_area_send) * n, hipMemcpyHostToDevice, c->stream));
			d_areas = c->calc.d_areas;
		}
		if (listener_area_pos) {
			GAS_HIP(c, hipMemcpyAsync(c->calc.d_lap, listener_area_pos, sizeof(float) * 3 * n_listeners * n, hipMemcpyHostToDevice, c->stream));
			d_lap = c->calc.d_lap;
		}
		if (out_reverb) {
			d_reverb = c->calc.d_reverb;
		}
	}
	GAS_HIP(c, gas_launch_calc_spatialization(c->stream, c->calc.d_cfgs, cfg_index ? c->calc.d_cfgidx : nullptr, d_poses, c->calc.d_listeners, n_listeners, c->calc.d_slots, n, c->st.params, c->st.was_further, d_out, d_areas, d_lap, d_reverb, c->st.hrtf_blend));
	if (mem == GAS_MEM_HOST && out_params) {
		GAS_HIP(c, hipMemcpyAsync(out_params, c->calc.d_out, sizeof(gas_params) * n, hipMemcpyDeviceToHost, c->stream));
	}
	if (mem == GAS_MEM_HOST && out_reverb) {
		GAS_HIP(c, hipMemcpyAsync(out_reverb, c->calc.d_reverb, sizeof(gas_audio_frame) * 4 * n, hipMemcpyDeviceToHost, c->stream));
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
	std::lock_guard<std::mutex> lk(c->calc.mu);
	if (slots) {
		c->calc.stamp.next();
		for (uint32_t i = 0; i < n; i++) {
			if (c->calc.stamp.seen(slots[i])) {
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
	GAS_HIP(c, alloc_once(c, c->calc.d_rooms, GAS_MAX_ROOMS));
	GAS_HIP(c, hipMemcpyAsync(c->calc.d_rooms, rooms, sizeof(gas_room) * n_rooms, hipMemcpyHostToDevice, c->stream));
	GAS_HIP(c, hipMemcpyAsync(c->calc.d_listeners, listener, sizeof(gas_listener), hipMemcpyHostToDevice, c->stream));
	if (slots) {
		GAS_HIP(c, hipMemcpyAsync(c->calc.d_slots, slots, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
	}
	if (room_index) { // config indices and room indices never travel in the same call
		GAS_HIP(c, hipMemcpyAsync(c->calc.d_cfgidx, room_index, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
	}
	const gas_source_pose *d_poses = poses;
	gas_er_taps *d_taps = out_taps;
	if (mem == GAS_MEM_HOST) {
		GAS_HIP(c, alloc_once(c, c->calc.d_poses, c->cfg.max_sources));
		GAS_HIP(c, hipMemcpyAsync(c->calc.d_poses, poses, sizeof(gas_source_pose) * n, hipMemcpyHostToDevice, c->stream));
		d_poses = c->calc.d_poses;
		if (out_taps) { // staged in the read-back buffer of gas_calc_spatialization's rows: a gas_er_taps is half a row
			static_assert(sizeof(gas_er_taps) <= sizeof(gas_params), "gas_er_taps are staged in calc.d_out");
			GAS_HIP(c, alloc_once(c, c->calc.d_out, c->cfg.max_sources));
			d_taps = reinterpret_cast<gas_er_taps *>(c->calc.d_out);
		}
	}
	GAS_HIP(c, gas_launch_calc_er(c->stream, c->calc.d_rooms, room_index ? c->calc.d_cfgidx : nullptr, d_poses, c->calc.d_listeners, c->calc.d_slots, n, c->cfg.er_ring_frames - c->cfg.frames, c->cfg.mix_rate, slots ? c->st.params : nullptr, d_taps));
	if (mem == GAS_MEM_HOST && out_taps) {
		GAS_HIP(c, hipMemcpyAsync(out_taps, d_taps, sizeof(gas_er_taps) * n, hipMemcpyDeviceToHost, c->stream));
	}
	GAS_HIP(c, hipStreamSynchronize(c->stream)); // the host staging arrays are the caller's
	return GAS_OK;
}

} // extern "C"
