// gas_ctx_conv.hip -- the bus convolvers of include/gas_amd.h (gas_ctx_reserve_conv, gas_conv_*; k_conv.hip) and the
// impulse responses built on the device from box rooms (gas_conv_ir_from_room*; k_room_ir.hip, k_room_bands.hip,
// k_room_tail.hip) and from rooms bounded by planes (gas_conv_ir_from_planes; k_room_planes.hip).
#include "gas_ctx_priv.h"

extern "C" {

#define GAS_CONV_MAX_IR_TAPS (1u << 20)

static void conv_release(gas_ctx *c) {
	c->mem.drop(c->conv.pool.ring);
	c->mem.drop(c->conv.pool.prev);
	c->mem.drop(c->conv.pool.ypart);
	c->mem.drop(c->conv.w1024);
	c->mem.drop(c->conv.h_in);
	c->mem.drop(c->conv.h_out);
	c->mem.drop(c->conv.d_in);
	c->mem.drop(c->conv.d_out);
	c->conv.pool = gas_conv_pool{};
	c->conv.count = 0;
	c->conv.max_taps = 0;
	c->conv.inst.clear();
	c->conv.free.clear();
	c->conv.irs.clear();
}

// The instance's ring and previous block become zeros in stream order: x[t] = 0 for every earlier t.
static hipError_t conv_zero(gas_ctx *c, uint32_t conv) {
	const size_t ring = (size_t)2 * c->conv.pool.K * GAS_CONV_BINS;
	const hipError_t e = hipMemsetAsync(c->conv.pool.ring + conv * ring, 0, ring * sizeof(float2), c->stream);
	return e != hipSuccess ? e : hipMemsetAsync(c->conv.pool.prev + (size_t)conv * 2 * 512, 0, 2 * 512 * sizeof(float), c->stream);
}

static bool conv_live(const gas_ctx *c, uint32_t conv) {
	return conv < c->conv.count && c->conv.inst[conv].used;
}

static bool conv_ir_live(const gas_ctx *c, uint32_t ir) {
	return ir < c->conv.irs.size() && c->conv.irs[ir].H != nullptr;
}

// The fade in progress ends in state B: A's IR is no longer named, B's reference becomes the state's.
static void conv_fade_land(gas_ctx *c, ConvInst &k) {
	c->conv.irs[k.ir].users--;
	k.ir = k.to.ir;
	k.dry = k.to.dry;
	k.wet = k.to.wet;
	k.fade_n = k.fade_pos = 0;
}

// gas_conv_set_ir, gas_conv_set_levels: a fade in progress ends at once in state B and a pending target is dropped.
static void conv_fade_end(gas_ctx *c, ConvInst &k) {
	if (k.fade_n) {
		conv_fade_land(c, k);
	}
	if (k.pending_n) {
		c->conv.irs[k.pending.ir].users--;
		k.pending_n = 0;
	}
}

int gas_ctx_reserve_conv(gas_ctx *c, uint32_t convolvers, uint32_t max_ir_taps) {
	if (!c || convolvers > GAS_MAX_CONVOLVERS || max_ir_taps > GAS_CONV_MAX_IR_TAPS || (convolvers == 0) != (max_ir_taps == 0)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	for (const auto &k : c->conv.inst) {
		if (k.used) {
			return GAS_ERR_INVALID_ARGUMENT;
		}
	}
	for (const auto &ir : c->conv.irs) {
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
		gas_conv_pool &p = c->conv.pool;
		p.K = K;
		p.max_chunks = gas_conv_max_chunks(K);
		GAS_HIP(c, c->mem.alloc(p.ring, (size_t)convolvers * 2 * K * GAS_CONV_BINS));
		GAS_HIP(c, c->mem.alloc(p.prev, (size_t)convolvers * 2 * 512));
		// two rows (ears) per named instance and two more per fading one: 96 rows of max_chunks spectra of 4 KiB,
		// 393 216 max_chunks bytes
		GAS_HIP(c, c->mem.alloc(p.ypart, (size_t)GAS_MAX_CONVOLVERS * 4 * p.max_chunks * GAS_CONV_BINS));
		GAS_HIP(c, c->mem.alloc(c->conv.w1024, 512));
		const size_t stage = (size_t)GAS_MAX_CONVOLVERS * F;
		GAS_HIP(c, c->mem.alloc(c->conv.h_in, stage, Mem::PINNED));
		GAS_HIP(c, c->mem.alloc(c->conv.h_out, stage, Mem::PINNED));
		GAS_HIP(c, c->mem.alloc(c->conv.d_in, stage));
		GAS_HIP(c, c->mem.alloc(c->conv.d_out, stage));
		float2 w[512];
		gas_make_w1024(w);
		GAS_HIP(c, hipMemcpyAsync(c->conv.w1024, w, sizeof(w), hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, hipStreamSynchronize(c->stream));
		p.w1024 = c->conv.w1024;
		return GAS_OK;
	}();
	if (rc != GAS_OK) {
		conv_release(c);
		return rc;
	}
	c->conv.count = convolvers;
	c->conv.max_taps = max_ir_taps;
	c->conv.inst.assign(convolvers, ConvInst{});
	c->conv.free.reserve(convolvers);
	for (uint32_t s = convolvers; s-- > 0;) {
		c->conv.free.push_back(s);
	}
	return GAS_OK;
}

// The common end of gas_conv_ir_load and gas_conv_ir_from_room: d_ir [channels][taps] is on the device, in the context's
// stream order.  Allocates the partition spectra, transforms, waits (the caller may free d_ir) and enters the IR in the
// table at the lowest free id.  A failure leaves no IR.
static int conv_ir_register(gas_ctx *c, const float *d_ir, uint32_t channels, uint32_t taps, uint32_t *out_ir) {
	const uint32_t F = c->cfg.frames;
	ConvIr rec;
	rec.channels = channels;
	rec.taps = taps;
	rec.k_ir = (taps + F - 1) / F;
	GAS_HIP(c, c->mem.alloc(rec.H, (size_t)channels * rec.k_ir * GAS_CONV_BINS));
	hipError_t e = gas_launch_conv_ir(c->stream, d_ir, channels, taps, F, c->d_tw, c->conv.pool.w1024, rec.H);
	e = e != hipSuccess ? e : hipStreamSynchronize(c->stream);
	if (e != hipSuccess) {
		c->mem.drop(rec.H);
		GAS_HIP(c, e);
	}
	uint32_t id = 0;
	while (id < c->conv.irs.size() && c->conv.irs[id].H) {
		id++;
	}
	if (id == c->conv.irs.size()) {
		c->conv.irs.push_back(rec);
	} else {
		c->conv.irs[id] = rec;
	}
	*out_ir = id;
	return GAS_OK;
}

int gas_conv_ir_load(gas_ctx *c, const float *ir, uint32_t channels, uint32_t taps, uint32_t *out_ir) {
	if (!c || !ir || !out_ir || (channels != 1 && channels != 2 && channels != 4) || taps == 0) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (c->conv.count == 0) {
		return GAS_ERR_UNSUPPORTED_CHAIN;
	}
	if (taps > c->conv.max_taps) {
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

int gas_conv_ir_free(gas_ctx *c, uint32_t ir) {
	if (!c) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (!conv_ir_live(c, ir)) {
		return GAS_ERR_BAD_SLOT;
	}
	if (c->conv.irs[ir].users != 0) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	GAS_TRY(flush_deferred(c));
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, hipStreamSynchronize(c->stream)); // calls still queued may read the spectra
	c->mem.drop(c->conv.irs[ir].H);
	c->conv.irs[ir] = ConvIr{};
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
		*out_channels = c->conv.irs[ir].channels;
	}
	if (out_taps) {
		*out_taps = c->conv.irs[ir].taps;
	}
	return GAS_OK;
}

int gas_conv_create(gas_ctx *c, uint32_t ir, uint32_t *out_conv) {
	if (!c || !out_conv) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (c->conv.count == 0) {
		return GAS_ERR_UNSUPPORTED_CHAIN;
	}
	if (!conv_ir_live(c, ir)) {
		return GAS_ERR_BAD_SLOT;
	}
	if (c->conv.free.empty()) {
		return GAS_ERR_OUT_OF_SLOTS;
	}
	const uint32_t id = c->conv.free.back();
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	GAS_HIP(c, conv_zero(c, id)); // zeroed when it changes hands
	c->conv.free.pop_back();
	ConvInst &k = c->conv.inst[id];
	k = ConvInst{};
	k.used = true;
	k.ir = ir;
	k.pos = c->conv.pool.K - 1;
	c->conv.irs[ir].users++;
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
	conv_fade_end(c, c->conv.inst[conv]); // releases every IR the instance names
	c->conv.irs[c->conv.inst[conv].ir].users--;
	c->conv.inst[conv].used = false;
	c->conv.free.push_back(conv);
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
	ConvInst &k = c->conv.inst[conv];
	k.pos = c->conv.pool.K - 1;
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
	conv_fade_end(c, c->conv.inst[conv]);
	c->conv.irs[c->conv.inst[conv].ir].users--;
	c->conv.inst[conv].ir = ir;
	c->conv.irs[ir].users++;
	return GAS_OK;
}

int gas_conv_set_levels(gas_ctx *c, uint32_t conv, float dry, float wet) {
	if (!c || !std::isfinite(dry) || !std::isfinite(wet)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (!conv_live(c, conv)) {
		return GAS_ERR_BAD_SLOT;
	}
	conv_fade_end(c, c->conv.inst[conv]);
	c->conv.inst[conv].dry = dry;
	c->conv.inst[conv].wet = wet;
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
	ConvInst &k = c->conv.inst[conv];
	ConvTarget t;
	t.ir = ir;
	t.dry = dry;
	t.wet = wet;
	c->conv.irs[ir].users++;
	if (k.fade_n) { // waits for the fade in progress; the latest target wins
		if (k.pending_n) {
			c->conv.irs[k.pending.ir].users--;
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
	const ConvInst &k = c->conv.inst[conv];
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
	const uint32_t K = c->conv.pool.K;
	gas_conv_call call{};
	for (uint32_t i = 0; i < n; i++) {
		const ConvInst &k = c->conv.inst[convs[i]];
		const ConvIr &ir = c->conv.irs[k.ir];
		gas_conv_entry &e = call.e[i];
		e.H = ir.H;
		e.slot = convs[i];
		e.pos = k.pos + 1 == K ? 0 : k.pos + 1;
		e.k_ir = ir.k_ir;
		e.mode = gas_conv_mode(ir.channels);
		e.dry = k.dry;
		e.wet = k.wet;
		if (k.fade_n) { // call fade_pos of fade_n: frame i has s = (float)(fade_pos F + i) * (1.0f / (float)(fade_n F))
			const ConvIr &irb = c->conv.irs[k.to.ir];
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
			GAS_HIP(c, gas_launch_conv(c->stream, call, n, c->conv.pool, c->d_tw, in, out, F));
			return GAS_OK;
		}
		// host memory: the previous host-memory call returned after its copies, so the staging is free
		std::memcpy(c->conv.h_in, in, bytes);
		GAS_HIP(c, hipMemcpyAsync(c->conv.d_in, c->conv.h_in, bytes, hipMemcpyHostToDevice, c->stream));
		GAS_HIP(c, gas_launch_conv(c->stream, call, n, c->conv.pool, c->d_tw, c->conv.d_in, c->conv.d_out, F));
		GAS_HIP(c, hipMemcpyAsync(c->conv.h_out, c->conv.d_out, bytes, hipMemcpyDeviceToHost, c->stream));
		GAS_HIP(c, hipStreamSynchronize(c->stream));
		std::memcpy(out, c->conv.h_out, bytes);
		return GAS_OK;
	}();
	if (rc != GAS_OK) {
		return fail(rc);
	}
	for (uint32_t i = 0; i < n; i++) {
		ConvInst &k = c->conv.inst[convs[i]];
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

// What gas_conv_ir_from_planes refuses in a descriptor's plain fields; a normal's length and where the points lie are the
// plan's to refuse.  Planes beyond n_planes and the listener's fields other than origin and basis column 0 are not read.
static bool room_planes_desc_ok(const gas_room_planes &d) {
	if (d.n_planes == 0 || d.n_planes > GAS_ROOM_MAX_PLANES || d.max_order == 0 || d.max_order > GAS_ROOM_PLANES_MAX_ORDER || d.min_order > d.max_order) {
		return false;
	}
	bool ok = d.speed_of_sound > 0.0f && std::isfinite(d.speed_of_sound) && d.level >= 0.0f && std::isfinite(d.level) && d.ear_spacing >= 0.0f && std::isfinite(d.ear_spacing);
	for (uint32_t j = 0; j < d.n_planes; j++) {
		const gas_room_plane &w = d.planes[j];
		ok = ok && std::isfinite(w.normal[0]) && std::isfinite(w.normal[1]) && std::isfinite(w.normal[2]) && std::isfinite(w.offset) && w.reflectance >= 0.0f && w.reflectance <= 1.0f;
	}
	for (int a = 0; a < 3; a++) {
		ok = ok && std::isfinite(d.source[a]) && std::isfinite(d.listener.origin[a]) && std::isfinite(d.listener.basis[a][0]);
	}
	return ok;
}

// The HRIR set of gas_conv_ir_from_room_hrtf, as the caller passed it.
struct RoomIrSet {
	const float *hrir;
	uint32_t n_az, n_el, taps;
};

// What the two *_bands calls refuse in a gas_room_bands; entries beyond n_bands (n_bands - 1 crossovers) are not read.
static bool room_bands_ok(const gas_room_bands &b, float rate) {
	if (b.n_bands == 0 || b.n_bands > GAS_ROOM_MAX_BANDS || b.reserved != 0) {
		return false;
	}
	bool ok = b.n_bands == 1 || ((b.filter_taps & 1u) && b.filter_taps >= 3 && b.filter_taps <= GAS_ROOM_BAND_FILTER_MAX_TAPS);
	float below = 0.0f;
	for (uint32_t i = 0; i + 1 < b.n_bands; i++) { // the comparisons are false for a NaN
		ok = ok && b.crossover_hz[i] > below && (double)b.crossover_hz[i] < (double)rate / 2.0;
		below = b.crossover_hz[i];
	}
	for (uint32_t i = 0; i < b.n_bands; i++) {
		for (int w = 0; w < 6; w++) {
			ok = ok && b.reflectance[i][w] >= 0.0f && b.reflectance[i][w] <= 1.0f;
		}
		ok = ok && b.air_db_per_m[i] >= 0.0f && std::isfinite(b.air_db_per_m[i]);
	}
	return ok;
}

// The common end of every generated IR: d_ir [channels][taps] is being written in the context's stream order.  out_ir:
// it is registered (which waits for the stream); out_taps: it is copied back.  At least one of the two is given.
static int conv_ir_deliver(gas_ctx *c, const float *d_ir, uint32_t channels, uint32_t taps, float *out_taps, uint32_t *out_ir) {
	const size_t n = (size_t)channels * taps;
	if (out_ir) { // waits for the stream
		uint32_t id = 0;
		GAS_TRY(conv_ir_register(c, d_ir, channels, taps, &id));
		if (out_taps) {
			const hipError_t e = hipMemcpy(out_taps, d_ir, n * sizeof(float), hipMemcpyDeviceToHost);
			if (e != hipSuccess) { // no IR and nothing reported: the caller's out_ir keeps its value
				c->mem.drop(c->conv.irs[id].H);
				c->conv.irs[id] = ConvIr{};
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

// A generator's launches inside the bracket of gas_profile_enable, where they count as a callback's dominant launch.
// (A template has C++ linkage, whatever surrounds it.)
extern "C++" {
template <class Launches>
static int conv_ir_bracketed(gas_ctx *c, Launches launches) {
	const bool timed = c->prof.room();
	if (timed) {
		GAS_HIP(c, c->prof.begin(c->stream));
	}
	GAS_TRY(launches());
	if (timed) {
		GAS_HIP(c, c->prof.end(c->stream));
	}
	return GAS_OK;
}
}

// The common body of the box-room calls once everything is validated and the plan is made: tables, temporaries,
// the generator's launches inside the profile bracket, registration and read-back.  set == nullptr: k_room_ir with
// `channels` receivers; otherwise k_room_ir_hrtf, two ears.  bands == nullptr: the plain calls, one pass whose scaled
// taps are the result; otherwise one such pass per band with that band's reflectances, each into its own sums, and
// k_room_bands_combine over them writes the result.  tail != nullptr (with bands): the *_diffuse calls -- `plan` is
// the lattice's, made for K1 taps (0: no lattice pass), its passes go into sums of their own, [passes][channels][K1],
// and k_room_tail mixes them into the sums of tail->taps taps that the combine reads.
static int conv_ir_from_plan(gas_ctx *c, const gas_room_ir &desc, const gas_room_ir_plan &plan, uint32_t channels, const RoomIrSet *set, const gas_room_bands *bands, const gas_room_tail_plan *tail, float *out_taps, uint32_t *out_ir) {
	const uint32_t taps = tail ? tail->taps : plan.taps;
	const uint32_t passes = bands ? bands->n_bands : 1u;
	const size_t per_pass = gas_room_ir_table_doubles(plan);
	gas_room_bands_plan bp{};
	std::vector<double> tables, filt;
	try {
		tables.resize(per_pass * passes);
		if (bands) {
			bp.bands = passes;
			bp.channels = channels;
			bp.taps = taps;
			bp.level = plan.level;
			bp.L = passes == 1 ? 1u : bands->filter_taps;
			bp.D = (bp.L - 1u) / 2u;
			bp.Lp = (bp.L + GAS_ROOM_BANDS_FILTER_STEP - 1u) / GAS_ROOM_BANDS_FILTER_STEP * GAS_ROOM_BANDS_FILTER_STEP;
			for (uint32_t b = 0; b < passes; b++) {
				bp.lambda[b] = 2.302585092994046 / 20.0 * (double)bands->air_db_per_m[b] * plan.c / plan.rate;
			}
			filt.resize((size_t)passes * bp.Lp);
			gas_room_bands_fill_filters(*bands, plan.rate, bp, filt.data());
		}
	} catch (const std::bad_alloc &) {
		c->last_err = "gas_conv_ir_from_room: out of host memory for the reflectance tables";
		return GAS_ERR_DEVICE;
	}
	if (bands) {
		gas_room_ir d = desc;
		for (uint32_t b = 0; b < passes; b++) {
			std::memcpy(d.room.reflectance, bands->reflectance[b], sizeof(d.room.reflectance));
			gas_room_ir_fill_tables(d, plan, tables.data() + per_pass * b);
		}
	} else {
		gas_room_ir_fill_tables(desc, plan, tables.data());
	}
	if (out_ir) { // the pure generator leaves queued callbacks where they are: it touches nothing of theirs
		GAS_TRY(flush_deferred(c));
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	const size_t n = (size_t)channels * taps, n_lat = (size_t)channels * plan.taps;
	Mem tmp; // frees the buffers on every way out
	double *d_tables = nullptr, *d_filt = nullptr;
	long long *d_acc = nullptr, *d_lat = nullptr; // what the combine reads; what the lattice passes write
	float *d_ir = nullptr, *d_hrir = nullptr;
	GAS_HIP(c, tmp.alloc(d_tables, tables.size()));
	GAS_HIP(c, tmp.alloc(d_acc, n * passes));
	if (!tail) {
		d_lat = d_acc;
	} else if (n_lat != 0) {
		GAS_HIP(c, tmp.alloc(d_lat, n_lat * passes));
	}
	GAS_HIP(c, tmp.alloc(d_ir, n));
	GAS_HIP(c, hipMemcpy(d_tables, tables.data(), tables.size() * sizeof(double), hipMemcpyHostToDevice)); // complete on return
	if (bands) {
		GAS_HIP(c, tmp.alloc(d_filt, filt.size()));
		GAS_HIP(c, hipMemcpy(d_filt, filt.data(), filt.size() * sizeof(double), hipMemcpyHostToDevice));
	}
	if (set) {
		const size_t floats = (size_t)set->n_az * set->n_el * 2 * set->taps;
		GAS_HIP(c, tmp.alloc(d_hrir, floats));
		GAS_HIP(c, hipMemcpy(d_hrir, set->hrir, floats * sizeof(float), hipMemcpyHostToDevice));
	}
	GAS_TRY(conv_ir_bracketed(c, [&]() -> int {
		for (uint32_t b = 0; b < passes && n_lat != 0; b++) { // in stream order: a band's scaled taps in d_ir (n_lat <= n of them) are overwritten by the next writer
			if (set) {
				GAS_HIP(c, gas_launch_room_ir_hrtf(c->stream, plan, desc, d_tables + per_pass * b, d_hrir, set->n_az, set->n_el, set->taps, d_lat + n_lat * b, d_ir));
			} else {
				GAS_HIP(c, gas_launch_room_ir(c->stream, plan, d_tables + per_pass * b, d_lat + n_lat * b, d_ir));
			}
		}
		if (tail) {
			GAS_HIP(c, gas_launch_room_tail(c->stream, *tail, d_lat, d_acc));
		}
		if (bands) {
			GAS_HIP(c, gas_launch_room_bands_combine(c->stream, bp, d_acc, d_filt, d_ir));
		}
		return GAS_OK;
	}));
	return conv_ir_deliver(c, d_ir, channels, taps, out_taps, out_ir);
}

// Which of the box-room calls of one name this is: it decides which of `bands` and `tail` must be there.
enum RoomCall { ROOM_PLAIN, ROOM_BANDS, ROOM_DIFFUSE };

// The *_diffuse calls' two plans once the descriptor's plain fields and the bands have passed: steps 1 - 3 of
// gas_conv_ir_from_room_diffuse.  `receivers` is the lattice's (1 for the HRTF call), `channels` the result's.  `lattice`
// is made for K1 taps, so its cell check is; with K1 == 0 only its geometry (the points inside the box, d0) is wanted, and
// it is made from a descriptor whose box cannot be refused for its size.  False for what either plan refuses.
static bool room_tail_plans(const gas_room_ir &desc, const gas_room_bands &bands, const gas_room_tail &tail, uint32_t receivers, uint32_t channels, uint32_t taps, float rate, gas_room_ir_plan &lattice, gas_room_tail_plan &tp) {
	uint32_t K0 = 0, K1 = 0;
	if (!gas_room_tail_marks(tail, (double)rate, taps, K0, K1)) {
		return false;
	}
	gas_room_ir d = desc;
	if (K1 == 0) {
		d.ear_spacing = 0.0f;
		d.min_order = 0;
		d.max_order = 1;
	}
	return gas_room_ir_make_plan(d, receivers, K1, rate, lattice) && gas_room_tail_make_plan(lattice, bands, tail, channels, taps, K0, K1, tp);
}

// What every generator checks once its arguments are there: registering (out_ir) needs a reserve, and `taps` must fit
// that reserve, or GAS_CONV_MAX_IR_TAPS for the pure generator.
static int conv_ir_room_for(const gas_ctx *c, uint32_t taps, const uint32_t *out_ir) {
	if (out_ir && c->conv.count == 0) {
		return GAS_ERR_UNSUPPORTED_CHAIN;
	}
	if (taps > (out_ir ? c->conv.max_taps : (uint32_t)GAS_CONV_MAX_IR_TAPS)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	return GAS_OK;
}

// The six box-room calls: `call` says which of the three names, so that a NULL bands or tail is refused by the calls
// that need it.  set == nullptr: the plain calls, `channels` receivers.  Otherwise the *_hrtf calls: one receiver (the
// listener; ear_spacing is not read) heard through the set, and two channels whatever `channels` says.
static int conv_ir_from_room_any(gas_ctx *c, const gas_room_ir *desc, RoomCall call, const gas_room_bands *bands, const gas_room_tail *tail, const RoomIrSet *set, uint32_t channels, uint32_t taps, float *out_taps, uint32_t *out_ir) {
	const bool banded = call != ROOM_PLAIN;
	if (!c || !desc || (banded && !bands) || (call == ROOM_DIFFUSE && !tail) || (!out_taps && !out_ir) || (set ? !set->hrir : channels != 1 && channels != 2) || taps == 0) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (set && (set->n_az == 0 || set->n_el == 0 || (uint64_t)set->n_az * set->n_el > 65536u || set->taps == 0 || set->taps > GAS_HRTF_TAPS)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	GAS_TRY(conv_ir_room_for(c, taps, out_ir));
	const uint32_t receivers = set ? 1u : channels;
	if (set) {
		channels = 2;
	}
	gas_room_ir_plan plan;
	gas_room_tail_plan tp;
	if (!room_ir_desc_ok(*desc, !set) || (banded && !room_bands_ok(*bands, c->cfg.mix_rate))) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (call == ROOM_DIFFUSE ? !room_tail_plans(*desc, *bands, *tail, receivers, channels, taps, c->cfg.mix_rate, plan, tp) : !gas_room_ir_make_plan(*desc, receivers, taps, c->cfg.mix_rate, plan)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	const size_t floats = set ? (size_t)set->n_az * set->n_el * 2 * set->taps : 0;
	for (size_t i = 0; i < floats; i++) {
		if (!(std::fabs(set->hrir[i]) <= 4.0f)) { // not finite, or a tap could pass 4 v per image: the int64 sums' bound
			return GAS_ERR_INVALID_ARGUMENT;
		}
	}
	return conv_ir_from_plan(c, *desc, plan, channels, set, bands, call == ROOM_DIFFUSE ? &tp : nullptr, out_taps, out_ir);
}

int gas_conv_ir_from_room(gas_ctx *c, const gas_room_ir *desc, uint32_t channels, uint32_t taps, float *out_taps, uint32_t *out_ir) {
	return conv_ir_from_room_any(c, desc, ROOM_PLAIN, nullptr, nullptr, nullptr, channels, taps, out_taps, out_ir);
}

int gas_conv_ir_from_room_hrtf(gas_ctx *c, const gas_room_ir *desc, const float *hrir, uint32_t n_az, uint32_t n_el, uint32_t hrir_taps, uint32_t taps, float *out_taps, uint32_t *out_ir) {
	const RoomIrSet set{hrir, n_az, n_el, hrir_taps};
	return conv_ir_from_room_any(c, desc, ROOM_PLAIN, nullptr, nullptr, &set, 2, taps, out_taps, out_ir);
}

int gas_conv_ir_from_room_bands(gas_ctx *c, const gas_room_ir *desc, const gas_room_bands *bands, uint32_t channels, uint32_t taps, float *out_taps, uint32_t *out_ir) {
	return conv_ir_from_room_any(c, desc, ROOM_BANDS, bands, nullptr, nullptr, channels, taps, out_taps, out_ir);
}

int gas_conv_ir_from_room_hrtf_bands(gas_ctx *c, const gas_room_ir *desc, const gas_room_bands *bands, const float *hrir, uint32_t n_az, uint32_t n_el, uint32_t hrir_taps, uint32_t taps, float *out_taps, uint32_t *out_ir) {
	const RoomIrSet set{hrir, n_az, n_el, hrir_taps};
	return conv_ir_from_room_any(c, desc, ROOM_BANDS, bands, nullptr, &set, 2, taps, out_taps, out_ir);
}

int gas_conv_ir_from_room_diffuse(gas_ctx *c, const gas_room_ir *desc, const gas_room_bands *bands, const gas_room_tail *tail, uint32_t channels, uint32_t taps, float *out_taps, uint32_t *out_ir) {
	return conv_ir_from_room_any(c, desc, ROOM_DIFFUSE, bands, tail, nullptr, channels, taps, out_taps, out_ir);
}

int gas_conv_ir_from_room_hrtf_diffuse(gas_ctx *c, const gas_room_ir *desc, const gas_room_bands *bands, const gas_room_tail *tail, const float *hrir, uint32_t n_az, uint32_t n_el, uint32_t hrir_taps, uint32_t taps, float *out_taps, uint32_t *out_ir) {
	const RoomIrSet set{hrir, n_az, n_el, hrir_taps};
	return conv_ir_from_room_any(c, desc, ROOM_DIFFUSE, bands, tail, &set, 2, taps, out_taps, out_ir);
}

// The planes road has no tables: the plan carries the planes, so its temporaries are the sums and the taps.  The
// bracket and the end are the box road's.
int gas_conv_ir_from_planes(gas_ctx *c, const gas_room_planes *desc, uint32_t channels, uint32_t taps, float *out_taps, uint32_t *out_ir) {
	if (!c || !desc || (!out_taps && !out_ir) || (channels != 1 && channels != 2) || taps == 0) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	GAS_TRY(conv_ir_room_for(c, taps, out_ir));
	gas_room_planes_plan plan;
	if (!room_planes_desc_ok(*desc) || !gas_room_planes_make_plan(*desc, channels, taps, c->cfg.mix_rate, plan)) {
		return GAS_ERR_INVALID_ARGUMENT;
	}
	if (out_ir) { // the pure generator leaves queued callbacks where they are: it touches nothing of theirs
		GAS_TRY(flush_deferred(c));
	}
	GAS_HIP(c, hipSetDevice(c->cfg.device));
	const size_t n = (size_t)channels * taps;
	Mem tmp; // frees the buffers on every way out
	long long *d_acc = nullptr;
	float *d_ir = nullptr;
	GAS_HIP(c, tmp.alloc(d_acc, n));
	GAS_HIP(c, tmp.alloc(d_ir, n));
	GAS_TRY(conv_ir_bracketed(c, [&]() -> int {
		GAS_HIP(c, gas_launch_room_planes(c->stream, plan, d_acc, d_ir));
		return GAS_OK;
	}));
	return conv_ir_deliver(c, d_ir, channels, taps, out_taps, out_ir);
}

} // extern "C"
