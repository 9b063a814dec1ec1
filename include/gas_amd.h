/*
 * gas_amd.h -- C ABI of the MI355X-native many-source spatializer.
 *
 * This is the drop-in boundary for ONE path of BuzzLord/godot-audio-spatializer:
 * the per-audio-callback work of AudioSpatializerInstance::_mix_from_playback_list
 * (audio_spatializer.cpp:326-471) and the plugin DSP it dispatches to
 * (audio_spatializer_3d.cpp:491-609, audio_spatializer_effect.cpp:33-77), batched
 * over every active source in one launch group.  Plain pointers and sizes only;
 * no exceptions cross it and nothing aborts: every entry returns 0 or a negative
 * gas_status, mirroring the reference's ERR_FAIL_* "log and return" style
 * (SURVEY.md section 5).  All file:line citations are in the reference tree.
 *
 * Threading contract (same split as audio_spatializer.h:135-138):
 *   - gas_params_publish*, gas_bus_routes_publish : physics thread, may run concurrently with the audio thread.
 *   - gas_source_alloc, gas_source_free : any thread, concurrently with the audio thread (instantiate_playback_data runs
 *     on the physics thread, audio_spatializer.cpp:69; playback data is released wherever its last reference drops).
 *     The slot allocator takes a lock; a free takes effect at the audio thread's next block boundary; a slot is
 *     handed to the audio thread by the caller (the first callback whose list names it), never before alloc returned.
 *   - gas_process_block*, gas_process_frames_1, gas_mix_channel_1, gas_source_set_draining, gas_source_bind_stream,
 *     gas_stream_positions, gas_sidechain_set : audio thread only, one caller at a time, never re-entrant per context.
 *   - everything else      : one thread at a time and not concurrently with the audio-thread entries -- the main
 *     thread while audio is stopped, or the audio thread itself between callbacks.
 */
#ifndef GAS_AMD_H
#define GAS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAS_ABI_VERSION 2 /* 2: gas_profile grew (callbacks_per_launch, bytes_per_callback_formula); pause / position / effect kinds */

/* audio_spatializer.h:47-52 */
#define GAS_MAX_CHANNELS_PER_BUS 4
#define GAS_LOOKAHEAD_BUFFER_SIZE 64
#define GAS_MAX_BUSES_PER_PLAYBACK 6

/* NEW (no reference counterpart): sizes of the HRTF / early-reflection effects. */
#define GAS_HRTF_TAPS 256
#define GAS_ER_TAPS 8
#define GAS_MAX_EFFECTS 4
#define GAS_MAX_SIDECHAINS 8 /* key blocks a context holds for the compressor's sidechain (gas_sidechain_set) */

typedef struct gas_ctx gas_ctx;

/* [ENGINE] AudioFrame: two interleaved f32 (left, right), 8 bytes. */
typedef struct gas_audio_frame {
	float left, right;
} gas_audio_frame;

typedef enum gas_status {
	GAS_OK = 0,
	GAS_ERR_INVALID_ARGUMENT = -1,
	GAS_ERR_OUT_OF_SLOTS = -2,
	GAS_ERR_BAD_SLOT = -3,
	GAS_ERR_FRAME_COUNT = -4, /* audio_spatializer.cpp:522 "Unexpected frame count" */
	GAS_ERR_NO_HRTF = -5,
	GAS_ERR_UNSUPPORTED_CHAIN = -6,
	GAS_ERR_DEVICE = -7, /* a HIP call failed; gas_last_device_error() has the text */
	GAS_ERR_NO_DEVICE = -8,
	GAS_ERR_OUT_OF_MEMORY = -9,
	GAS_ERR_KIND_MISMATCH = -10,
	GAS_ERR_BAD_CHANNEL = -11, /* audio_spatializer.cpp:521 "Unexpected channel" */
	GAS_ERR_NO_PARAMS = -12, /* audio_spatializer.cpp:330 parameters.is_null() */
} gas_status;

/* Which AudioSpatializerInstance flavour a source slot belongs to. */
typedef enum gas_source_kind {
	GAS_KIND_3D_MIX = 0, /* AudioSpatializer3D, mix_channel_mode=true : _mix_channel per channel pair (audio_spatializer_3d.cpp:554-609) */
	GAS_KIND_3D_PROCESS = 1, /* AudioSpatializer3D, mix_channel_mode=false: _process_frames (audio_spatializer_3d.cpp:491-552) */
	GAS_KIND_EFFECT = 2, /* AudioSpatializerEffect / AudioSpatializerHRTF: effect chain (audio_spatializer_effect.cpp:33-77) */
} gas_source_kind;

typedef enum gas_effect_kind {
	GAS_FX_HIGHSHELF = 1, /* [ENGINE] AudioEffectHighShelfFilter, FILTER_6DB (gd_spatializer.gd:14-19) */
	GAS_FX_EARLY_REFLECTIONS = 2, /* NEW: 8 stereo delay taps from a per-source ring */
	GAS_FX_HRTF = 3, /* NEW: mono downmix -> gain ramp -> 256-tap HRIR pair, overlap-save FFT */
	/* audio_spatializer_effect.cpp:79-88 instantiates ANY AudioEffect; these are the engine's other one-biquad filters
	 * ([ENGINE] AudioEffectFilter subclasses at FILTER_6DB = one AudioFilterSW stage per ear, coefficients snapped per
	 * block) and AudioEffectAmplify.  Their settings are per playback and chain position: gas_fx_settings. */
	GAS_FX_LOWPASS = 4, /* [ENGINE] AudioEffectLowPassFilter */
	GAS_FX_HIGHPASS = 5, /* [ENGINE] AudioEffectHighPassFilter */
	GAS_FX_BANDPASS = 6, /* [ENGINE] AudioEffectBandPassFilter */
	GAS_FX_NOTCH = 7, /* [ENGINE] AudioEffectNotchFilter */
	GAS_FX_LOWSHELF = 8, /* [ENGINE] AudioEffectLowShelfFilter */
	GAS_FX_AMPLIFY = 9, /* [ENGINE] AudioEffectAmplify: volume ramp previous -> current volume_db across the block */
	/* The engine's first nonlinear and dynamics kinds; settings per playback and chain position: gas_fx_dyn_settings.
	 * (10 is not assigned: an effect kind the library does not know is GAS_ERR_INVALID_ARGUMENT / _UNSUPPORTED_CHAIN.) */
	GAS_FX_DISTORTION = 11, /* [ENGINE] AudioEffectDistortion: per-ear one-pole split, the low band shaped by `mode` */
	GAS_FX_COMPRESSOR = 12, /* [ENGINE] AudioEffectCompressor: stereo-linked detector on the playback's own frames or on a sidechain key (gas_sidechain_set), one gain per frame */
	/* The engine's time-domain kinds with long per-instance memory ("lines", reserved with gas_ctx_reserve_fx_lines);
	 * settings per playback and chain position: gas_fx_line_settings. */
	GAS_FX_DELAY = 13, /* [ENGINE] AudioEffectDelay: two panned taps and a low-passed feedback echo, ears independent */
	GAS_FX_REVERB = 14, /* [ENGINE] AudioEffectReverb: predelay echo, 8 combs, 4 allpasses per ear (Freeverb tunings) */
	/* The engine's graphic equalisers: one unity-peak resonator per band and ear, summed with a gain per band (state in
	 * "banks", reserved with gas_ctx_reserve_fx_eq); settings per playback and chain position: gas_fx_eq_settings.
	 * (15 is not assigned.) */
	GAS_FX_EQ6 = 16, /* [ENGINE] AudioEffectEQ6: bands at 32, 100, 320, 1000, 3200, 10000 Hz */
	GAS_FX_EQ10 = 17, /* [ENGINE] AudioEffectEQ10: bands at 31.25 Hz and every octave up to 16 kHz */
	GAS_FX_EQ21 = 18, /* [ENGINE] AudioEffectEQ21: bands at 22 Hz to 22 kHz, half an octave apart */
	/* The engine's modulation kinds (state in "lines" and "banks", reserved with gas_ctx_reserve_fx_mod); settings per
	 * playback and chain position: gas_fx_mod_settings. */
	GAS_FX_CHORUS = 19, /* [ENGINE] AudioEffectChorus: up to 4 LFO-modulated taps of a stereo ring, each low-passed and panned */
	GAS_FX_PHASER = 20, /* [ENGINE] AudioEffectPhaser: six first-order allpasses per ear with feedback, swept by one LFO */
	/* The engine's stereo kinds: no recurrence over frames.  Panner and limiter hold no state; every stereo enhance holds
	 * one mono delay "ring" (gas_ctx_reserve_fx_stereo).  Settings per playback and chain position: gas_fx_stereo_settings. */
	GAS_FX_PANNER = 21, /* [ENGINE] AudioEffectPanner: each ear keeps its own share and takes the other's remainder */
	GAS_FX_STEREO_ENHANCE = 22, /* [ENGINE] AudioEffectStereoEnhance: side gain, then a delayed right ear or a delayed mid as +/- surround */
	GAS_FX_LIMITER = 23, /* [ENGINE] AudioEffectLimiter: make-up gain, soft clip above -soft_clip_db, hard ceiling */
	/* The engine's AudioEffectFilter of any subclass at any slope, and AudioEffectBandLimitFilter: 1 .. 4 cascaded
	 * AudioFilterSW stages per ear (state in "banks", reserved with gas_ctx_reserve_fx_filter); settings per playback and
	 * chain position: gas_fx_filter_settings.  Kinds 1 and 4 .. 8 stay the one-stage forms they are. */
	GAS_FX_FILTER = 24, /* [ENGINE] AudioEffectFilter: `type` at FILTER_6DB .. FILTER_24DB */
} gas_effect_kind;

/* gas_fx_filter_settings.type: which AudioEffectFilter subclass (the AudioFilterSW mode it selects) */
#define GAS_FILTER_LOWPASS 0
#define GAS_FILTER_HIGHPASS 1
#define GAS_FILTER_BANDPASS 2
#define GAS_FILTER_NOTCH 3
#define GAS_FILTER_LOWSHELF 4
#define GAS_FILTER_HIGHSHELF 5
#define GAS_FILTER_BANDLIMIT 6 /* [ENGINE] AudioEffectBandLimitFilter: `resonance` is the band's other edge (> 0) */
/* gas_fx_filter_settings.db: [ENGINE] AudioEffectFilter::FilterDB, db + 1 cascaded stages */
#define GAS_FILTER_6DB 0
#define GAS_FILTER_12DB 1
#define GAS_FILTER_18DB 2
#define GAS_FILTER_24DB 3

/* [ENGINE] AudioEffectDistortion::Mode */
#define GAS_DISTORTION_CLIP 0
#define GAS_DISTORTION_ATAN 1
#define GAS_DISTORTION_LOFI 2
#define GAS_DISTORTION_OVERDRIVE 3
#define GAS_DISTORTION_WAVESHAPE 4

typedef enum gas_mem {
	GAS_MEM_HOST = 0, /* host pointers; the call copies in/out and returns when the result is in *out */
	GAS_MEM_DEVICE = 1, /* device pointers on the context's GPU; the call only enqueues on the context stream */
} gas_mem;

/* Mirrors module initialisation (register_types.cpp:40) + the AudioServer facts the
 * reference reads at run time (mix rate audio_spatializer_3d.cpp:506, channel count
 * audio_spatializer.cpp:176, the fixed 512-frame mix step). */
typedef struct gas_config {
	uint32_t struct_size; /* sizeof(gas_config) */
	int32_t device; /* HIP device ordinal */
	uint32_t max_sources; /* slots of device-resident SpatializerPlaybackData */
	uint32_t frames; /* F: frames per callback, fixed for the context (audio_spatializer.cpp:522); multiple of 128, <= 512 */
	uint32_t channel_count; /* C: AudioServer channel pairs, 1..4 (audio_spatializer.cpp:172-179) */
	float mix_rate; /* AudioServer::get_mix_rate(), e.g. 48000 */
	uint32_t er_ring_frames; /* early-reflection ring length per source (power of two, 0 = effect unavailable) */
	uint32_t flags; /* GAS_FLAG_* */
} gas_config;

/* gas_config.flags */
/* The reference computes every playback's output peak but only reads it once the stream has ended
 * (audio_spatializer.cpp:464-469).  With this flag HRTF sources that are NOT marked draining are summed
 * in the frequency domain (one forward FFT per source, inverse FFTs per workgroup) and report
 * peak = +inf ("not measured", never passes the gate); the mix is unchanged.  Without it every source
 * reports its exact peak, as the reference computes it.  "HRTF sources": chains [HRTF] and [ER, HRTF], and any other
 * chain whose LAST effect is the HRTF when the context runs that stage in the one-launch kernel (no cross-fade /
 * direction-run flags); every other chain reports exact peaks with or without the flag (they cost nothing there). */
#define GAS_FLAG_PEAKS_DRAINING_ONLY 1u
/* NEW: when an HRTF source's direction differs from the one of its previous callback, render the
 * block with both HRIRs and blend old -> new with t = i/F (the analogue of the per-block volume lerp,
 * audio_spatializer_3d.cpp:591-592) instead of switching at the block boundary. */
#define GAS_FLAG_HRTF_CROSSFADE 2u
/* HRTF sources whose hrtf_dir repeats can share one forward FFT (sum_s Z_s H[d] = FFT(sum_s z_s) H[d]).
 * GAS_FLAG_DIRECTION_RUNS: the caller keeps sources with equal hrtf_dir adjacent in the callback's list (as far as
 * it likes: any list is correct); frequency-domain sources then sum each run in the time domain before one FFT
 * (measured 15-19 % less kernel time at 8 sources per direction; 4-5 % MORE on a list without runs, hence a flag).
 * GAS_FLAG_DIRECTION_ORDER: the library builds the grouping itself (a device counting sort per 8192-source segment,
 * re-run after every parameter publish or list change); implies _RUNS.  Pays only when parameters are published
 * much less often than callbacks run.  Results are identical up to f32 summation order; neither
 * flag has an effect together with GAS_FLAG_HRTF_CROSSFADE. */
#define GAS_FLAG_DIRECTION_ORDER 4u
/* Throughput mode for callers that queue many callbacks (offline rendering, benchmarks): the final sum of the
 * per-workgroup partial mixes of gas_process_block(GAS_MEM_DEVICE) is not launched as its own kernel; it is carried
 * out by otherwise idle waves of the NEXT callback's HRTF kernel (one dispatch per callback instead of two).  `out`
 * of such a call is complete only after the next gas_process_block on this context, gas_ctx_join_outputs(),
 * gas_ctx_synchronize(), or any GAS_MEM_HOST / single-instance call -- each in the context's stream order; peaks
 * are not deferred.  Keep `out` valid and unread until then.  Applies to contexts with channel_count == 1 whose
 * callback contains HRTF sources; other callbacks are summed immediately.  Same operations in the same order:
 * results are bitwise identical to the ordered mode.  A synchronous audio callback gains nothing from it. */
#define GAS_FLAG_PIPELINED_MIX 8u
#define GAS_FLAG_DIRECTION_RUNS 16u /* see GAS_FLAG_DIRECTION_ORDER */
/* XCD-affine processing order for plain [HRTF] callbacks (>= 2048 sources): after every parameter publish or list
 * change one small launch (k_xcd_order) permutes the callback's sources so that each of the GPU's eight XCDs (own L2
 * each) keeps working on the same eighth of the HRIR spectra table.  MEASURED (profiles/r02_notes.md): L2 fills drop
 * from 1.46x to 1.05x of the algorithmic bytes at 65536 sources, but the kernel gains only 4 % (the rows are then read
 * in scattered instead of list order) and the ordering launch costs more than that -- so it is OFF unless asked for;
 * kept because it answers what the excess traffic costs.  The mix is the same sum in another (still deterministic)
 * order: results agree to f32 rounding, not bitwise, with the unordered launch. */
#define GAS_FLAG_XCD_ORDER 32u
/* With GAS_FLAG_PIPELINED_MIX, for callers that queue callbacks faster than they consume them (offline rendering,
 * benchmarks): consecutive gas_process_block(GAS_MEM_DEVICE) calls of an unchanged plain-[HRTF] list run as ONE launch
 * per `depth` callbacks (k_hrtf_multi: no dispatch gap between them, a callback's epilogue under the next one's
 * stream; depth 2 unless gas_ctx_set_batch_depth says otherwise).  A call only records its arguments until the batch is
 * full; the call that fills it enqueues all of them.  Same operations in the same order: results are bitwise those of
 * the unbatched mode.  What changes for the caller:
 *  - `src`, `peaks` and device-published parameter rows of a call must stay valid and unmodified until `depth - 1`
 *    further gas_process_block calls on this context (or gas_ctx_join_outputs / gas_ctx_synchronize) have returned;
 *  - `out` is complete only after gas_ctx_join_outputs / gas_ctx_synchronize (or any ordered call), in stream order;
 *  - every call waiting for its batch or its deferred sum needs ITS OWN `out` (and `peaks`) buffer: the sums of the
 *    queued callbacks are written out of call order (a block's sum rides in a later launch, the join sums everything
 *    pending in one parallel launch), so two queued calls that share an `out` race; the unbatched mode's
 *    "last call wins" does not hold here;
 *  - every entry of the context must be called from ONE thread (the recorded calls are run by whoever comes next:
 *    anything that changes what they must see -- a new list, host-published parameters, frees, any other entry that
 *    enqueues work -- first runs them, exactly as the unbatched mode would have);
 *  - callbacks that do not qualify (other source kinds, < 2048 sources, 2 or more channel pairs, streams, cross-fade,
 *    direction or HRIR-interpolation flags) run as before. */
#define GAS_FLAG_BATCHED_LAUNCH 64u
/* NEW: every HRTF stage of the context convolves with a weighted sum of up to four rows of the HRIR
 * set instead of the one row hrtf_dir names: H = sum_i weight[i] * H[dir[i]] over the slot's gas_hrtf_blend row (added
 * in f32, in index order, before the spectral product; the HRTF stage is linear in the HRIR, so this is the weighted
 * sum of the single-direction renders).  Rows come from gas_hrtf_blend_publish or from gas_calc_spatialization, which
 * then writes the bilinear weights of the grid cell around the source next to hrtf_dir.  A slot whose row is all zero
 * (every slot when it is allocated) has no blend: it renders hrtf_dir at weight 1, through the same code.  HRTF sources
 * of such a context run in k_hrtf_ols (the kernel the cross-fade uses), never in k_hrtf_uni / k_hrtf_multi, so their
 * mixes agree with an unflagged context's to rounding, not to the bit.  Without the flag nothing changes anywhere.
 * Cost per context: 32 bytes of device memory per slot of max_sources for the blend table (0.26 MB at 8192 slots, 2 MB
 * at 65 536, 260 MB at 8.1 M) plus, once a row has been published, 32 bytes of pinned host memory per slot for the
 * upload; the host mirror is 32 bytes per slot of ordinary memory.  gas_ctx_create refuses the flag
 * (GAS_ERR_INVALID_ARGUMENT) together with GAS_FLAG_HRTF_CROSSFADE (that flag fades from ONE
 * old direction; fading from an old blend to a new one is GAS_FLAG_HRTF_BLEND_FADE) and with GAS_FLAG_DIRECTION_RUNS, GAS_FLAG_DIRECTION_ORDER and GAS_FLAG_XCD_ORDER (they group or order
 * sources by their ONE direction). */
#define GAS_FLAG_HRTF_INTERPOLATE 128u
/* NEW: fade between successive blends, valid only together with GAS_FLAG_HRTF_INTERPOLATE.  The blend row is read once
 * per callback, so without this flag the filter of a moving source switches at every block boundary where its row
 * changed; with it the block is rendered with the old and the new blend and lerped across the block, the way
 * GAS_FLAG_HRTF_CROSSFADE lerps between two single directions (mix_channel's volume lerp, audio_spatializer_3d.cpp:591-592).
 *  - A playback's EFFECTIVE ROW for a callback is what the HRTF stage derives from its gas_hrtf_blend row: the entries
 *    of non-zero weight moved to the front in index order, directions clamped as hrtf_dir is (>= the set's dirs -> 0),
 *    the remaining entries zero; the all-zero row becomes { hrtf_dir, 1 }.
 *  - The stage renders  y[i] = t * (sum_k w_new,k * x conv h[dir_new,k])[i] + (1 - t) * (sum_k w_old,k * x conv
 *    h[dir_old,k])[i],  t = (float)i * (1 / F),  where `old` is the effective row of the LAST CALLBACK THAT PROCESSED
 *    THIS SLOT and x is the stage's gained mono input; the hrtf_gain ramp is unchanged and independent of the fade.
 *  - A slot with no old row renders the new row alone: the first callback after gas_source_alloc, after
 *    gas_source_reset, and after a free plus re-alloc of the slot.  A playback left out of a callback's list keeps its
 *    old row.
 *  - "Changed" means that any of the eight 32-bit words of the effective row differs from the stored one.  A source
 *    whose row did not change loads no table row beyond those of its blend.
 *  - Rows written on the device by gas_calc_spatialization fade exactly like published ones: the comparison is made
 *    in the HRTF kernel, nothing is read back.  Peaks are those of the faded output.
 * Every road a GAS_FLAG_HRTF_INTERPOLATE context takes is covered (plain [HRTF] and [EARLY_REFLECTIONS, HRTF],
 * frequency-domain and exact-peak, PCM streams, staged chains, bus callbacks); batched launches do not qualify and a
 * pipelined callback is summed at once, as with the blend alone.  Cost per context: another 32 bytes of device memory
 * per slot of max_sources (the stored effective rows).  gas_ctx_create refuses the flag (GAS_ERR_INVALID_ARGUMENT)
 * without GAS_FLAG_HRTF_INTERPOLATE and with each flag GAS_FLAG_HRTF_INTERPOLATE is refused with.  Contexts without
 * the flag behave exactly as before. */
#define GAS_FLAG_HRTF_BLEND_FADE 256u
/* NEW: fade the early-reflection taps between callbacks.  The rule is stated at gas_params::er_delay.  The flag changes
 * early-reflection stages and nothing else: the chain [EARLY_REFLECTIONS] and every staged chain's early-reflection
 * stage fade; [EARLY_REFLECTIONS, HRTF] runs as a staged chain (the early-reflection stage writes rows, the HRTF stage
 * reads them as it does behind any other stage: two launches and a row round trip in place of the fused kernel, whatever
 * GAS_UNI_ER says), because the fused kernels have no fading form.  A staged chain with an early-reflection stage is
 * refused by gas_source_alloc (GAS_ERR_UNSUPPORTED_CHAIN) on a context with er_ring_frames == 0; a flagged context
 * always has a ring, so a flagged [EARLY_REFLECTIONS, HRTF] is accepted wherever the unflagged one is.  Bus, stream,
 * host and multi-device entries run their early-reflection stages through the same launches.  gas_ctx_create refuses
 * the flag (GAS_ERR_INVALID_ARGUMENT) with er_ring_frames == 0 and with no other flag.  Cost per context: 68 bytes of
 * device memory per slot of max_sources (the stored rows and the "has rendered" word).  Contexts without the flag
 * behave exactly as before. */
#define GAS_FLAG_ER_TAP_FADE 512u

/* SpatializerParameters (spatializer_parameters.h:39-67) + SpatializerParameters3D
 * (audio_spatializer_3d.h:61-83) as one 128-byte POD, plus the per-block effect
 * parameters a _process_effects hook would push (audio_spatializer_effect.cpp:90-92,
 * gd_spatializer_instance.gd:125-127).  bus_volumes stay on the host: they only feed
 * AudioServer via get_bus_map (audio_spatializer.cpp:274-324). */
typedef struct gas_params {
	float mix_volumes[GAS_MAX_CHANNELS_PER_BUS][2]; /* must describe 4 channel pairs, spatializer_parameters.cpp:45 */
	float pitch_scale; /* consumed by the host-side sampler only (audio_spatializer.cpp:375) */
	float linear_attenuation; /* high-shelf gain, audio_spatializer_3d.h:67 */
	float attenuation_filter_cutoff_hz; /* audio_spatializer_3d.h:68, default 5000 */
	uint32_t update_parameters; /* spatializer_parameters.h:50, host-side only */
	float hrtf_gain; /* NEW: linear gain ramped across the block before the HRIR */
	uint32_t hrtf_dir; /* NEW: HRIR direction index */
	float fx_shelf_gain; /* GAS_FX_HIGHSHELF gain (linear) */
	float fx_shelf_cutoff_hz; /* GAS_FX_HIGHSHELF cutoff */
	float er_gain[GAS_ER_TAPS]; /* NEW */
	uint32_t er_delay[GAS_ER_TAPS]; /* NEW: 1 .. er_ring_frames - frames.  A value above er_ring_frames - frames acts as
	                                  * er_ring_frames - frames (the oldest frame the ring holds); 0 adds the frame itself.
	                                  * NEW, GAS_FLAG_ER_TAP_FADE (no counterpart in the engine).  A playback's EFFECTIVE TAP ROW
	                                  * for a callback is 16 words: er_gain[8] as stored, then min(er_delay[k], er_ring_frames -
	                                  * frames) -- so a raw delay outside the range equals its clamped value.  The context keeps,
	                                  * per slot, the row the early-reflection stage LAST RENDERED WITH and whether it has rendered
	                                  * at all (an all-zero row is a legal tap set).  With Y_row[f] = x[f] + sum_k g[k] * x[f -
	                                  * d[k]] (tap order, f32, the playback's one history):
	                                  *  - no old row, or old and new row bitwise equal: y = Y_new, bit for bit what a context
	                                  *    without the flag stores;
	                                  *  - otherwise y[f] = t * Y_new[f] + (1 - t) * Y_old[f], t = (float)f * (1 / frames): frame 0
	                                  *    is all old, the next callback starts all new (GAS_FLAG_HRTF_BLEND_FADE's ramp);
	                                  *  - then the new row becomes the slot's old row.
	                                  * A playback left out of a callback (not listed, paused) keeps ring, position and old row, and
	                                  * fades from the taps it last rendered with when it returns.  gas_source_reset, and a free
	                                  * plus re-alloc of the slot, forget the old row: the first block after them does not fade.
	                                  * Peaks are those of the faded output. */
} gas_params;

/* Settings of the GAS_FX_LOWPASS .. GAS_FX_AMPLIFY effects of one playback, by chain position (what a script sets on
 * the AudioEffect resources from _process_effects, gd_spatializer_instance.gd:125-127).  Position j is read only when
 * effect j of the playback's chain is one of those kinds.  A slot that never got settings has the engine's resource
 * defaults: cutoff 2000 Hz, resonance 0.5, gain 1, volume 0 dB. */
typedef struct gas_fx_settings {
	float filter_cutoff_hz[GAS_MAX_EFFECTS]; /* [ENGINE] AudioEffectFilter::cutoff */
	float filter_resonance[GAS_MAX_EFFECTS]; /* [ENGINE] AudioEffectFilter::resonance */
	float filter_gain[GAS_MAX_EFFECTS]; /* [ENGINE] AudioEffectFilter::gain (linear; shelf kinds) */
	float amplify_volume_db[GAS_MAX_EFFECTS]; /* [ENGINE] AudioEffectAmplify::volume_db */
} gas_fx_settings;

/* Settings of the GAS_FX_DISTORTION / GAS_FX_COMPRESSOR effects of one playback, by chain position like gas_fx_settings:
 * position j is read only when effect j of the playback's chain is one of those kinds.  Read once per block (no ramps).
 * A slot that never got settings has the engine's resource defaults, given per field.  The compressor's `sidechain`
 * bus is compressor_sidechain[j]: 0 (the default) detects on the playback's own frames, k in 1 .. GAS_MAX_SIDECHAINS
 * detects on key block k - 1 of the context (gas_sidechain_set); the gain is applied to the playback's own frames either
 * way, and the state (rundb) is the same one whatever the value is. */
typedef struct gas_fx_dyn_settings {
	int32_t distortion_mode[GAS_MAX_EFFECTS]; /* GAS_DISTORTION_*, default CLIP */
	float distortion_pre_gain_db[GAS_MAX_EFFECTS]; /* default 0 */
	float distortion_keep_hf_hz[GAS_MAX_EFFECTS]; /* default 16000 */
	float distortion_drive[GAS_MAX_EFFECTS]; /* 0 .. 1, default 0 */
	float distortion_post_gain_db[GAS_MAX_EFFECTS]; /* default 0 */
	float compressor_threshold_db[GAS_MAX_EFFECTS]; /* default 0 */
	float compressor_ratio[GAS_MAX_EFFECTS]; /* > 0, default 4 */
	float compressor_gain_db[GAS_MAX_EFFECTS]; /* makeup gain, default 0 */
	float compressor_attack_us[GAS_MAX_EFFECTS]; /* > 0, default 20 */
	float compressor_release_ms[GAS_MAX_EFFECTS]; /* > 0, default 250 */
	float compressor_mix[GAS_MAX_EFFECTS]; /* default 1 */
	uint32_t compressor_sidechain[GAS_MAX_EFFECTS]; /* 0 .. GAS_MAX_SIDECHAINS, default 0: no sidechain */
} gas_fx_dyn_settings;

/* Settings of the GAS_FX_DELAY / GAS_FX_REVERB effects of one playback, by chain position like gas_fx_dyn_settings:
 * position j is read only when effect j of the playback's chain is one of those kinds.  Read once per block.  A slot's
 * settings start at the engine's resource defaults, given per field, when the slot is allocated.  Ranges (the engine's
 * property ranges; gas_fx_line_settings_publish refuses anything outside them at any position): tap and feedback
 * delays 0 .. 1500 ms, pans -1 .. 1, lowpass 1 .. 16000 Hz, predelay 20 .. 500 ms, predelay feedback 0 .. 0.98, the
 * other reverb fields and delay_dry 0 .. 1, levels finite.  The *_active fields are on when not 0. */
typedef struct gas_fx_line_settings {
	float delay_dry[GAS_MAX_EFFECTS]; /* default 1 */
	int32_t delay_tap1_active[GAS_MAX_EFFECTS]; /* default 1 */
	float delay_tap1_ms[GAS_MAX_EFFECTS]; /* default 250 */
	float delay_tap1_level_db[GAS_MAX_EFFECTS]; /* default -6 */
	float delay_tap1_pan[GAS_MAX_EFFECTS]; /* default 0.2 */
	int32_t delay_tap2_active[GAS_MAX_EFFECTS]; /* default 1 */
	float delay_tap2_ms[GAS_MAX_EFFECTS]; /* default 500 */
	float delay_tap2_level_db[GAS_MAX_EFFECTS]; /* default -12 */
	float delay_tap2_pan[GAS_MAX_EFFECTS]; /* default -0.4 */
	int32_t delay_feedback_active[GAS_MAX_EFFECTS]; /* default 0 */
	float delay_feedback_ms[GAS_MAX_EFFECTS]; /* default 340 */
	float delay_feedback_level_db[GAS_MAX_EFFECTS]; /* default -6 */
	float delay_feedback_lowpass_hz[GAS_MAX_EFFECTS]; /* default 16000 */
	float reverb_predelay_ms[GAS_MAX_EFFECTS]; /* default 150 */
	float reverb_predelay_feedback[GAS_MAX_EFFECTS]; /* default 0.4 */
	float reverb_room_size[GAS_MAX_EFFECTS]; /* default 0.8 */
	float reverb_damping[GAS_MAX_EFFECTS]; /* default 0.5 */
	float reverb_spread[GAS_MAX_EFFECTS]; /* default 1 */
	float reverb_hipass[GAS_MAX_EFFECTS]; /* default 0 */
	float reverb_dry[GAS_MAX_EFFECTS]; /* default 1 */
	float reverb_wet[GAS_MAX_EFFECTS]; /* default 0.5 */
} gas_fx_line_settings;

/* Settings of the GAS_FX_EQ6 / GAS_FX_EQ10 / GAS_FX_EQ21 effects of one playback, by chain position, then band: position
 * j is read only when effect j of the playback's chain is one of those kinds; EQ6 reads bands 0..5, EQ10 bands 0..9.
 * Read once per block (no ramp).  A slot's settings start at 0 dB everywhere when it is allocated.  Range (the engine's
 * property range; gas_fx_eq_settings_publish refuses anything outside it or not finite, at any position and band, used
 * or not): -60 .. 24 dB. */
#define GAS_EQ_MAX_BANDS 21
typedef struct gas_fx_eq_settings {
	float band_gain_db[GAS_MAX_EFFECTS][GAS_EQ_MAX_BANDS];
} gas_fx_eq_settings;

/* Settings of the GAS_FX_CHORUS / GAS_FX_PHASER effects of one playback, by chain position (then voice for the
 * chorus's [GAS_MAX_EFFECTS][GAS_CHORUS_MAX_VOICES] arrays): position j is read only when effect j of the playback's
 * chain is one of those kinds.  Read once per block (no ramp).  A slot's settings start at the defaults below when it is
 * allocated.  Ranges (the engine's property ranges; gas_fx_mod_settings_publish refuses anything outside them or not
 * finite, at any position and voice, used or not) and defaults by voice 0, 1, 2, 3: */
#define GAS_CHORUS_MAX_VOICES 4
typedef struct gas_fx_mod_settings {
	int32_t chorus_voice_count[GAS_MAX_EFFECTS]; /* 1 .. 4, default 2 */
	float chorus_dry[GAS_MAX_EFFECTS]; /* 0 .. 1, default 1 */
	float chorus_wet[GAS_MAX_EFFECTS]; /* 0 .. 1, default 0.5 */
	float chorus_delay_ms[GAS_MAX_EFFECTS][GAS_CHORUS_MAX_VOICES]; /* 0 .. 50, default 15, 20, 12, 12 */
	float chorus_rate_hz[GAS_MAX_EFFECTS][GAS_CHORUS_MAX_VOICES]; /* 0.1 .. 20, default 0.8, 1.2, 1, 1 */
	float chorus_depth_ms[GAS_MAX_EFFECTS][GAS_CHORUS_MAX_VOICES]; /* 0 .. 20, default 2, 3, 0, 0 */
	float chorus_level_db[GAS_MAX_EFFECTS][GAS_CHORUS_MAX_VOICES]; /* -60 .. 24, default 0 */
	float chorus_cutoff_hz[GAS_MAX_EFFECTS][GAS_CHORUS_MAX_VOICES]; /* 1 .. 20500, default 8000, 8000, 16000, 16000; >= 16000: no low-pass */
	float chorus_pan[GAS_MAX_EFFECTS][GAS_CHORUS_MAX_VOICES]; /* -1 .. 1, default -0.5, 0.5, 0, 0 */
	float phaser_range_min_hz[GAS_MAX_EFFECTS]; /* 10 .. 10000, default 440 (min > max is legal) */
	float phaser_range_max_hz[GAS_MAX_EFFECTS]; /* 10 .. 10000, default 1600 */
	float phaser_rate_hz[GAS_MAX_EFFECTS]; /* 0.01 .. 20, default 0.5 */
	float phaser_feedback[GAS_MAX_EFFECTS]; /* 0.1 .. 0.9, default 0.7 */
	float phaser_depth[GAS_MAX_EFFECTS]; /* 0.1 .. 4, default 1 */
} gas_fx_mod_settings;

/* Settings of the GAS_FX_PANNER / GAS_FX_STEREO_ENHANCE / GAS_FX_LIMITER effects of one playback, by chain position:
 * position j is read only when effect j of the playback's chain is one of those kinds.  Read once per block (no ramp).
 * A slot's settings start at the defaults below when it is allocated.  Ranges (the engine's property ranges;
 * gas_fx_stereo_settings_publish refuses anything outside them or not finite, at any position, used or not): */
typedef struct gas_fx_stereo_settings {
	float panner_pan[GAS_MAX_EFFECTS]; /* -1 .. 1, default 0 */
	float enhance_pan_pullout[GAS_MAX_EFFECTS]; /* 0 .. 4, default 1 */
	float enhance_time_pullout_ms[GAS_MAX_EFFECTS]; /* 0 .. 50, default 0 */
	float enhance_surround[GAS_MAX_EFFECTS]; /* 0 .. 1, default 0 (> 0: the surround mode) */
	float limiter_ceiling_db[GAS_MAX_EFFECTS]; /* -20 .. -0.1, default -0.1 */
	float limiter_threshold_db[GAS_MAX_EFFECTS]; /* -30 .. 0, default 0 */
	float limiter_soft_clip_db[GAS_MAX_EFFECTS]; /* 0 .. 6, default 2 */
	float limiter_soft_clip_ratio[GAS_MAX_EFFECTS]; /* 3 .. 20, default 10 (carried; the engine's process never reads it) */
} gas_fx_stereo_settings;

/* Settings of the GAS_FX_FILTER effects of one playback, by chain position: position j is read only when effect j of the
 * playback's chain is GAS_FX_FILTER.  Read once per block: the engine's set_cutoff, set_gain, set_resonance,
 * set_stages(db + 1), then every processor snaps to the new coefficients (no ramp).  Stages at index db + 1 and above
 * are not run and keep their history, so `db` may change between blocks.  A slot's settings start at the defaults
 * below when it is allocated.  gas_fx_filter_settings_publish refuses, at any position, used or not: a `type` or `db`
 * that is none of the constants above, anything not finite or outside the engine's property ranges, and -- a deviation
 * from the engine, whose band-limit coefficients are NaN there -- GAS_FILTER_BANDLIMIT with resonance <= 0. */
typedef struct gas_fx_filter_settings {
	int32_t type[GAS_MAX_EFFECTS]; /* GAS_FILTER_*, default LOWPASS */
	int32_t db[GAS_MAX_EFFECTS]; /* GAS_FILTER_6DB .. _24DB, default 6 dB */
	float cutoff_hz[GAS_MAX_EFFECTS]; /* 1 .. 20500, default 2000 */
	float resonance[GAS_MAX_EFFECTS]; /* 0 .. 1, default 0.5 */
	float gain[GAS_MAX_EFFECTS]; /* 0 .. 4, default 1 (linear; the shelf types) */
	uint32_t reserved[12];
} gas_fx_filter_settings;

/* Per-kernel device timing collected with HIP events on the context stream. */
typedef struct gas_profile {
	uint64_t launches; /* timed launches of the dominant kernel since the last reset */
	double kernel_ms; /* sum of their durations */
	uint64_t bytes_per_launch; /* bytes the last timed launch had to move: SURVEY.md 8d's per-callback
	                            * formula for a one-callback launch; for a launch of K callbacks (GAS_FLAG_BATCHED_LAUNCH)
	                            * K x (frames + per-block parameters / peaks + partial mix) + the history rows once in and
	                            * once out when they stay in LDS between blocks (K times otherwise) + the HRIR table once */
	char kernel_name[64];
	uint32_t callbacks_per_launch; /* K of the last timed launch (1 unless batched) */
	uint32_t reserved;
	uint64_t bytes_per_callback_formula; /* SURVEY.md 8d's per-callback figure x K: what round 2 reported for batched launches */
} gas_profile;

/* ---- context ---------------------------------------------------------- */
int gas_abi_version(void);
int gas_ctx_create(const gas_config *cfg, gas_ctx **out_ctx);
void gas_ctx_destroy(gas_ctx *ctx);
/* Run on an existing HIP stream (hipStream_t) instead of the context's own. */
int gas_ctx_set_stream(gas_ctx *ctx, void *hip_stream);
int gas_ctx_synchronize(gas_ctx *ctx);
/* GAS_FLAG_BATCHED_LAUNCH: callbacks per launch, 1 (off) .. 16; takes effect with the next batch. */
int gas_ctx_set_batch_depth(gas_ctx *ctx, uint32_t depth);
/* GAS_FLAG_PIPELINED_MIX: enqueue the deferred sum of the last gas_process_block, so that work enqueued on the
 * context's stream after this call sees its `out`.  Non-blocking; no-op when nothing is pending. */
int gas_ctx_join_outputs(gas_ctx *ctx);
int gas_ctx_get_config(gas_ctx *ctx, gas_config *out); /* the configuration the context was created with */
const char *gas_strerror(int status);
const char *gas_last_device_error(gas_ctx *ctx);

/* ---- per-playback state: _instantiate_playback_data (audio_spatializer.cpp:69),
 * deferred delete (audio_spatializer.cpp:538-547) ------------------------ */
/* GAS_KIND_EFFECT chains (audio_spatializer_effect.cpp:33-77): up to GAS_MAX_EFFECTS of GAS_FX_*, in processing
 * order, with at most one EARLY_REFLECTIONS (needs cfg.er_ring_frames) and one HRTF per playback.  [], [HIGHSHELF],
 * [ER], [HRTF] and [ER, HRTF] run as one fused kernel; any other order or kind runs one launch per effect through
 * ping-pong row buffers, as the reference's loop does.  Everything else: GAS_ERR_UNSUPPORTED_CHAIN. */
int gas_source_alloc(gas_ctx *ctx, int kind, const int32_t *effects, uint32_t n_effects, uint32_t *out_slot);
int gas_source_free(gas_ctx *ctx, uint32_t slot); /* takes effect at the next block boundary */
int gas_source_reset(gas_ctx *ctx, uint32_t slot); /* zero the slot's DSP state (a restarted playback) */
/* has_frames cleared (audio_spatializer.cpp:398): from now on the host reads this source's peak.  Changing the
 * flag invalidates the cached slot list: pass `slots` to the next gas_process_block. */
int gas_source_set_draining(gas_ctx *ctx, uint32_t slot, int draining);

/* ---- set_spatializer_parameters (audio_spatializer.cpp:558-564): latest wins,
 * snapshotted once at the start of the next gas_process_block (:328) ------ */
int gas_params_publish(gas_ctx *ctx, uint32_t slot, const gas_params *params);
/* params_mem == GAS_MEM_DEVICE with slots == NULL addresses the slot list of the last gas_process_block in its row
 * order and is DEFERRED: the rows are read when the next gas_process_block (or any other entry that needs the table)
 * is enqueued, so the buffer must stay valid and unmodified on other streams until then. */
int gas_params_publish_batch(gas_ctx *ctx, const uint32_t *slots, const gas_params *params, uint32_t n, int params_mem);

/* Settings of the engine-effect kinds, host arrays; latest wins, snapshotted with the parameters at the start of the
 * next gas_process_block.  Physics thread, like gas_params_publish. */
int gas_fx_settings_publish(gas_ctx *ctx, const uint32_t *slots, const gas_fx_settings *settings, uint32_t n);
/* The same for gas_fx_dyn_settings: latest wins, snapshotted at the start of the next gas_process_block, physics thread.
 * A distortion_mode outside 0..4, a compressor ratio, attack or release that is not > 0, or a compressor_sidechain
 * above GAS_MAX_SIDECHAINS (at any position, used or not) is GAS_ERR_INVALID_ARGUMENT, and nothing of the call is taken. */
int gas_fx_dyn_settings_publish(gas_ctx *ctx, const uint32_t *slots, const gas_fx_dyn_settings *settings, uint32_t n);
/* The compressor's sidechain keys.  The context owns GAS_MAX_SIDECHAINS key blocks of cfg.frames AudioFrames in device
 * memory, allocated and zeroed by gas_ctx_create with the pinned staging the host form needs (nothing is allocated
 * here).  The call replaces the block of `key`; frames == NULL zeroes it (a silent key: over = 0, the compressor
 * releases).  With GAS_MEM_HOST `frames` has been consumed when the call returns: it is copied into the key's pinned
 * staging block and uploaded in stream order.  The call does not wait for that upload, but it does wait for the SAME
 * key's previous host upload if that one is still queued behind earlier work of the stream (device-memory callbacks
 * not yet finished): up to the GPU time of what is queued, nothing when the stream has caught up, as it has after any
 * GAS_MEM_HOST callback.  How often that happens in a running game has not been measured.  With GAS_MEM_DEVICE the call only
 * enqueues a device copy in the context's stream order, so the buffer must stay valid until that point of the stream
 * -- it may be the `out` of an earlier callback on the same stream, which is how one of the caller's own bus mixes
 * becomes a key.  Audio thread, between callbacks.  A key keeps its block until it is replaced: a callback with no
 * gas_sidechain_set in front of it detects on the same block again, and every compressor stage of every callback
 * enqueued after the call reads the new block.  Callbacks recorded or deferred before the call (GAS_FLAG_BATCHED_LAUNCH)
 * run first; their results are unchanged.  Keys are context state: gas_source_reset and gas_source_free do not touch
 * them.  key >= GAS_MAX_SIDECHAINS, a bad `mem` or ctx == NULL is GAS_ERR_INVALID_ARGUMENT, frame_count != cfg.frames
 * GAS_ERR_FRAME_COUNT, a HIP failure GAS_ERR_DEVICE; an error changes nothing.  A gas_multi caller sets keys per shard
 * (gas_multi_shard). */
int gas_sidechain_set(gas_ctx *ctx, uint32_t key, const gas_audio_frame *frames, uint32_t frame_count, int mem);
/* The same for gas_fx_line_settings: latest wins, snapshotted at the start of the next gas_process_block, physics
 * thread.  A value outside the ranges given at gas_fx_line_settings (at any position) is GAS_ERR_INVALID_ARGUMENT, and
 * nothing of the call is taken. */
int gas_fx_line_settings_publish(gas_ctx *ctx, const uint32_t *slots, const gas_fx_line_settings *settings, uint32_t n);
/* The same for gas_fx_eq_settings: latest wins, snapshotted at the start of the next gas_process_block, physics thread.
 * A gain outside -60 .. 24 dB or not finite (at any position and band) is GAS_ERR_INVALID_ARGUMENT, and nothing of the
 * call is taken. */
int gas_fx_eq_settings_publish(gas_ctx *ctx, const uint32_t *slots, const gas_fx_eq_settings *settings, uint32_t n);
/* The same for gas_fx_mod_settings: latest wins, snapshotted at the start of the next gas_process_block, physics
 * thread.  A value outside the ranges given at gas_fx_mod_settings or not finite (at any position and voice) is
 * GAS_ERR_INVALID_ARGUMENT, and nothing of the call is taken. */
int gas_fx_mod_settings_publish(gas_ctx *ctx, const uint32_t *slots, const gas_fx_mod_settings *settings, uint32_t n);
/* The same for gas_fx_stereo_settings: latest wins, snapshotted at the start of the next gas_process_block, physics
 * thread.  A value outside the ranges given at gas_fx_stereo_settings or not finite (at any position) is
 * GAS_ERR_INVALID_ARGUMENT, and nothing of the call is taken.  Needs no reservation: the device settings table, the
 * slot -> ring table and the staging buffers are allocated by gas_ctx_create, where gas_fx_settings' table is, whether
 * or not a chain ever holds one of the kinds.  Cost per context: 292 bytes of device memory (128 settings, 16 table,
 * 148 staging) and 148 bytes of pinned host memory per slot of max_sources -- 2.4 MB and 1.2 MB at 8192 slots, 19 MB
 * and 9.7 MB at 65 536, 2.4 GB and 1.2 GB at 8.1 M. */
int gas_fx_stereo_settings_publish(gas_ctx *ctx, const uint32_t *slots, const gas_fx_stereo_settings *settings, uint32_t n);
/* The same for gas_fx_filter_settings: latest wins, snapshotted at the start of the next gas_process_block, physics
 * thread.  Settings refused by the rules given at gas_fx_filter_settings (at any position) are
 * GAS_ERR_INVALID_ARGUMENT, and nothing of the call is taken. */
int gas_fx_filter_settings_publish(gas_ctx *ctx, const uint32_t *slots, const gas_fx_filter_settings *settings, uint32_t n);

/* ---- delay memory of the GAS_FX_DELAY / GAS_FX_REVERB instances ("lines") ---------------------------------------
 * Every GAS_FX_DELAY of a chain holds one delay line, every GAS_FX_REVERB one reverb line, from two device pools the
 * caller sizes here.  Main thread, never concurrently with gas_process_block (like gas_hrtf_load).  The call allocates
 * the pools, the slot -> line table, the device settings table and a pinned upload buffer; nothing is allocated on the
 * audio thread.  (0, 0) releases everything.  While any line is held (by an allocated slot, or a freed one before the
 * next block boundary) the call is GAS_ERR_INVALID_ARGUMENT.  reverb_lines > 0 needs lrint(0.02 mix_rate) >= frames and
 * lrint(0.025306122 mix_rate) >= frames (about 25.6 kHz at 512 frames), else GAS_ERR_INVALID_ARGUMENT.  With sr the
 * mix rate (f64), the bytes per line are:
 *   delay:  256 + 8 R + 8 ((int)(1.5 sr) + 1), R = the smallest power of two >= (int)(1.5 sr) + 513
 *           (about 1.5 MiB at 48 kHz);
 *   reverb: 256 + 4 sum over the two ears e of (echo + sum_k comb_k(e) + sum_k allpass_k(e)),
 *           echo = (int)(0.5 sr + 1), comb_k(e) = lrint(ct_k sr) + xs(e), allpass_k(e) = lrint(at_k sr) + xs(e),
 *           xs(0) = 0, xs(1) = lrint(0.000521 sr), ct / at the Freeverb tunings of DESIGN.md 3.5e (about 300 KiB);
 * each rounded up to a multiple of 256.  gas_source_alloc takes one line per such effect of the chain: with no pool
 * reserved it is GAS_ERR_UNSUPPORTED_CHAIN, with too few free lines GAS_ERR_OUT_OF_SLOTS (nothing taken).  Lines go
 * back with the slot at the next block boundary after gas_source_free; they are zeroed whenever they change hands and
 * by gas_source_reset.  A gas_multi caller reserves per shard (gas_multi_shard). */
int gas_ctx_reserve_fx_lines(gas_ctx *ctx, uint32_t delay_lines, uint32_t reverb_lines);

/* ---- state of the GAS_FX_EQ6 / _EQ10 / _EQ21 instances ("banks") -----------------------------------------------
 * Every equaliser of a chain holds one bank (2 ears x 21 bands x 4 floats, 672 bytes) from a device pool the caller
 * sizes here, with the same contract as gas_ctx_reserve_fx_lines: main thread, never concurrently with
 * gas_process_block; the pool, the slot -> bank table, the device settings table and a pinned upload buffer are
 * allocated here and nothing on the audio thread; 0 releases everything; while any bank is held the call is
 * GAS_ERR_INVALID_ARGUMENT.  gas_source_alloc takes one bank per equaliser of the chain: with no pool reserved it is
 * GAS_ERR_UNSUPPORTED_CHAIN, with too few free banks (or lines, for a chain that also holds a delay or reverb)
 * GAS_ERR_OUT_OF_SLOTS, and nothing is taken.  Banks go back with the slot at the next block boundary after
 * gas_source_free; they are zeroed whenever they change hands and by gas_source_reset.  The two reservations are
 * independent: neither call touches the other's pool.  A gas_multi caller reserves per shard (gas_multi_shard). */
int gas_ctx_reserve_fx_eq(gas_ctx *ctx, uint32_t eq_banks);

/* ---- state of the GAS_FX_CHORUS / GAS_FX_PHASER instances (chorus "lines", phaser "banks") ------------------------
 * Every chorus of a chain holds one chorus line, every phaser one phaser bank, from two device pools the caller sizes
 * here, with the same contract as gas_ctx_reserve_fx_lines: main thread, never concurrently with gas_process_block; the
 * pools, the slot -> line / bank table, the device settings table and a pinned upload buffer are allocated here and
 * nothing on the audio thread; (0, 0) releases everything; while any line or bank is held the call is
 * GAS_ERR_INVALID_ARGUMENT.  Bytes per instance, with sr the mix rate:
 *   chorus: 256 + 8 R, R = 1 << bitlength((int)(0.24 sr)) ring frames (16384 at 44.1 and 48 kHz, 32768 at 96 kHz);
 *   phaser: 64.
 * chorus_lines > 0 needs R >= lrint(0.05 sr) + 2 (int)(0.02 sr) + 12 + frames (the longest read plus one block), else
 * GAS_ERR_INVALID_ARGUMENT.  gas_source_alloc takes one line or bank per such effect of the chain: with neither pool
 * reserved it is GAS_ERR_UNSUPPORTED_CHAIN, with too few free lines or banks in any pool (these, the delay and reverb
 * lines, the EQ banks) GAS_ERR_OUT_OF_SLOTS, and nothing is taken.  Lines and banks go back with the slot at the next
 * block boundary after gas_source_free; they are zeroed whenever they change hands and by gas_source_reset.  The
 * reservation is independent of gas_ctx_reserve_fx_lines and gas_ctx_reserve_fx_eq: no call touches another's pools.
 * A gas_multi caller reserves per shard (gas_multi_shard). */
int gas_ctx_reserve_fx_mod(gas_ctx *ctx, uint32_t chorus_lines, uint32_t phaser_banks);

/* ---- delay memory of the GAS_FX_STEREO_ENHANCE instances ("rings") ------------------------------------------------
 * Every stereo enhance of a chain holds one ring from a device pool the caller sizes here, with the same contract as
 * gas_ctx_reserve_fx_mod: main thread, never concurrently with gas_process_block; the pool and the room of the pinned
 * upload buffer that names the rings to zero are allocated here and nothing on the audio thread (the slot -> ring
 * table and the device settings table exist from gas_ctx_create on: GAS_FX_PANNER and GAS_FX_LIMITER hold no state,
 * and chains of only those two and other stateless kinds need no reservation at all); 0 releases the pool; while any
 * ring is held the call is GAS_ERR_INVALID_ARGUMENT.  Bytes per ring, with sr the mix rate: 16 + 4 R,
 * R = 1 << bitlength((int)(0.052 sr)) mono frames (the engine's; 4096 at 44.1 and 48 kHz, 8192 at 96 kHz).  The kernel
 * writes a block into the ring after every read of its launch, so it needs only R >= frames (no two frames of a block
 * on one entry; R > (unsigned)(0.05 sr), the longest delay, always holds): enhance_rings > 0 with R < frames is
 * GAS_ERR_INVALID_ARGUMENT.  gas_source_alloc takes one ring per stereo enhance of the chain: with no pool reserved it
 * is GAS_ERR_UNSUPPORTED_CHAIN, with too few free entries in any pool the chain needs (these, the delay and reverb
 * lines, the EQ banks, the chorus lines, the phaser banks) GAS_ERR_OUT_OF_SLOTS, and nothing is taken.  Rings go back
 * with the slot at the next block boundary after gas_source_free; they are zeroed whenever they change hands and by
 * gas_source_reset.  The reservation is independent of gas_ctx_reserve_fx_lines, gas_ctx_reserve_fx_eq and
 * gas_ctx_reserve_fx_mod: no call touches another's pools.  A gas_multi caller reserves per shard (gas_multi_shard). */
int gas_ctx_reserve_fx_stereo(gas_ctx *ctx, uint32_t enhance_rings);

/* ---- state of the GAS_FX_FILTER instances ("banks") ----------------------------------------------------------------
 * Every GAS_FX_FILTER of a chain holds one bank ([4 stages][a1, a2, b1, b2][2 ears] floats, 128 bytes: the history of
 * the engine's four processors per ear) from a device pool the caller sizes here, with the same contract as
 * gas_ctx_reserve_fx_eq: main thread, never concurrently with gas_process_block; the pool, the slot -> bank table, the
 * device settings table and a pinned upload buffer are allocated here and nothing on the audio thread (a context that
 * never reserves pays nothing); 0 releases everything; while any bank is held the call is GAS_ERR_INVALID_ARGUMENT.
 * gas_source_alloc takes one bank per GAS_FX_FILTER of the chain: with no pool reserved it is
 * GAS_ERR_UNSUPPORTED_CHAIN, with too few free entries in any pool the chain needs (these, the delay and reverb lines,
 * the EQ banks, the chorus lines, the phaser banks, the rings) GAS_ERR_OUT_OF_SLOTS, and nothing is taken.  Banks go
 * back with the slot at the next block boundary after gas_source_free; they are zeroed whenever they change hands and
 * by gas_source_reset.  The reservation is independent of the other gas_ctx_reserve_fx_* calls: no call touches
 * another's pools.  A gas_multi caller reserves per shard (gas_multi_shard). */
int gas_ctx_reserve_fx_filter(gas_ctx *ctx, uint32_t banks);

/* ---- NEW AudioSpatializerHRTF resource: hrir is [dirs][2 ears][taps] f32, taps <= 256 */
int gas_hrtf_load(gas_ctx *ctx, const float *hrir, uint32_t dirs, uint32_t taps);

/* GAS_FLAG_HRTF_INTERPOLATE: the HRIR rows one playback's HRTF stage blends.  Entries with weight == 0 are ignored and
 * their dir is not read.  Weights are used as given, not normalised: they scale the output like hrtf_gain does.  The
 * all-zero row means "no blend": gas_params.hrtf_dir at weight 1. */
typedef struct gas_hrtf_blend {
	uint32_t dir[4];
	float weight[4];
} gas_hrtf_blend;
/* Host arrays, physics thread, latest wins; snapshotted with the parameters at the start of the next
 * gas_process_block* (like gas_fx_settings_publish).  GAS_ERR_INVALID_ARGUMENT, and nothing of the call is taken: a
 * context without GAS_FLAG_HRTF_INTERPOLATE; a weight that is negative or not finite; a dir >= the loaded set's
 * direction count on an entry with non-zero weight.  The direction check is made HERE, against the set loaded at the
 * time of the call; with no set loaded yet (or after a smaller set is loaded later) the kernel clamps an out-of-range
 * dir to direction 0, exactly as it clamps hrtf_dir.  gas_source_free returns the slot's row to all-zero at the next
 * block boundary; gas_source_reset leaves it (settings, not DSP state). */
int gas_hrtf_blend_publish(gas_ctx *ctx, const uint32_t *slots, const gas_hrtf_blend *blends, uint32_t n);
/* The same resource from a MEASURED set (what a SOFA file holds: M source positions x 2 receivers x N samples; parsing
 * netCDF / HDF5 is the caller's business, the loader takes the arrays).  positions is [m][2] = (azimuth, elevation) in
 * radians, azimuth from straight ahead (-Z) towards the right (+X), elevation up from the horizontal plane -- SOFA's
 * spherical convention is azimuth counter-clockwise in degrees: azimuth = -radians(sofa_azimuth).  hrir is
 * [m][2 ears][taps], taps <= 256 (shorter sets are zero-padded).  The set is regridded ON THE DEVICE onto the
 * az_steps x el_steps grid the library indexes directions with (hrtf_dir = elevation_index * az_steps + azimuth_index;
 * azimuth_index = round(az / 2pi * az_steps) mod az_steps, elevation_index = round((el + pi/2) / pi * (el_steps - 1)):
 * the cells gas_calc_spatialization writes): interpolation 0 takes the measurement nearest on the sphere, 1 blends the
 * three nearest with weights 1 / (angle + 1e-4) -- a time-domain blend, adequate for dense sets only.  out_hrir, when
 * non-NULL, receives the gridded set [az_steps * el_steps][2][256] (what gas_hrtf_load was then called with).  NEW, no
 * reference counterpart: parity unpinned.  Main thread, like gas_hrtf_load. */
int gas_hrtf_load_positions(gas_ctx *ctx, const float *positions, const float *hrir, uint32_t m, uint32_t taps, uint32_t az_steps, uint32_t el_steps, int interpolation, float *out_hrir);

/* ---- the hot path: body of _mix_from_playback_list (audio_spatializer.cpp:353-470)
 * for n sources at once.  src is [n][frames] AudioFrames, row i already holds the
 * 64-frame-delayed window of source slots[i] (audio_spatializer.cpp:367-378);
 * out is [C][frames] (C = channel_count for GAS_KIND_3D_MIX sources, else row 0 only
 * is non-zero) and is fully overwritten (zeros when n == 0, :335-343); peaks is
 * [n][2] = per-source max |L|, max |R| over its mixed output (:436-443,:453-460),
 * feeding the host's silence gate (:464-469).  slots == NULL reuses the previous
 * call's slot list (n must match).  On error the status is returned and, for host
 * memory, *out is zero-filled. */
int gas_process_block(gas_ctx *ctx, const gas_audio_frame *src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, float *peaks, int mem);

/* ---- several output buses ---------------------------------------------------------------------
 * In the reference every playback carries a bus_volumes dictionary (spatializer_parameters.h:39-67: <= 6 buses,
 * audio_spatializer.h:52) and AudioServer multiplies the frames a proxy returns by get_bus_map's per-channel-pair
 * factors for each of them (audio_spatializer.cpp:274-324).  AudioSpatializer3D fills it with the dry bus -- the
 * player's, or the Area3D's override -- at the output volume, and the area's reverb bus at reverb_volume
 * (audio_spatializer_3d.cpp:437-461).  For a mix-channel instance the dry factor is bus/mix = 1 and the send factor
 * is reverb_volume / mix_volume per channel pair and ear (0 where the mix volume is <= 0, :295-313).  Batched, that
 * is: every source names the bus its dry signal goes to and (optionally) a bus that receives it scaled by `send`;
 * one launch produces all buses:
 *     out[b][c][i] = sum over sources with dry_bus == b of y[c][i]  +  sum over sources with send_bus == b of y[c][i] * send[c]
 * (y = the source's mix_channel output for pair c).  GAS_KIND_3D_MIX sources only. */
#define GAS_MAX_BUSES GAS_MAX_BUSES_PER_PLAYBACK
#define GAS_MAX_MORE_SENDS (GAS_MAX_BUSES_PER_PLAYBACK - 2)
#define GAS_BUS_NONE 0xffffffffu
/* A playback reaches up to GAS_MAX_BUSES_PER_PLAYBACK buses (audio_spatializer.cpp:283-287 walks every key of
 * bus_volumes up to that many): the dry bus and up to five sends.  AudioSpatializer3D uses the dry bus and one send
 * (audio_spatializer_3d.cpp:437-461): the first two fields; a script subclass with more buses fills more_*.  A bus
 * named more than once receives the sum of its weights. */
typedef struct gas_bus_route {
	uint32_t dry_bus; /* index < n_buses of the call, or GAS_BUS_NONE */
	uint32_t send_bus; /* first send: index < n_buses, or GAS_BUS_NONE */
	float send[GAS_MAX_CHANNELS_PER_BUS][2]; /* bus_volume / mix_volume per channel pair and ear (gas_host_bus_map arithmetic) */
	uint32_t more_bus[GAS_MAX_MORE_SENDS]; /* further sends; GAS_BUS_NONE = unused */
	float more_send[GAS_MAX_MORE_SENDS][GAS_MAX_CHANNELS_PER_BUS][2];
} gas_bus_route;
/* Host arrays; latest wins, snapshotted at the next gas_process_block_buses.  A slot that never got a route is
 * {dry_bus 0, no send}.  Physics thread, like gas_params_publish. */
int gas_bus_routes_publish(gas_ctx *ctx, const uint32_t *slots, const gas_bus_route *routes, uint32_t n);
/* gas_process_block with out = [n_buses][C][frames] (1 <= n_buses <= GAS_MAX_BUSES).  Either every source is
 * GAS_KIND_3D_MIX (the mix-channel buses, fused into the biquad launch), or every source is a non-empty effect chain
 * on a one-pair context (the chains run staged -- per-source rows -- and the rows are mixed per bus with send[0]);
 * anything else is GAS_ERR_UNSUPPORTED_CHAIN.  Plain [HRTF] sources run fused, one launch per PAIR of buses (the second
 * bus's spectra sums in LDS), the last launch committing the playbacks' state.  slots == NULL reuses the previous call's
 * list (3D mix and fused [HRTF] forms).  Peaks are those of y (before any bus factor), as the reference's gate sees them
 * (audio_spatializer.cpp:436-443). */
int gas_process_block_buses(gas_ctx *ctx, const gas_audio_frame *src, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, uint32_t n_buses, float *peaks, int mem);

/* ---- convolution reverb for bus mixes ("convolvers") -------------------------------------------------------------
 * NEW: the engine has no counterpart (its buses are mixed and their effects run on the CPU; nothing in it convolves).
 * A convolver is one instance per bus and channel pair: it holds an impulse response h_e[0 .. T) per ear e and every
 * frame it has been given.  From an IR of one channel both ears use channel 0, from an IR of two channels ear e uses
 * channel e.  With x[t] the frames given to the instance, t counting on across its gas_conv_process calls and
 * x[t] = 0 for t < 0 (before its first call and before the first call after gas_conv_reset):
 *
 *     y_e[t] = dry * x_e[t] + wet * sum_{j=0}^{T-1} h_e[j] * x_e[t - j]
 *
 * With such an IR the ears are independent (no cross-feed).  NEW: an IR of four channels ("true stereo", the form
 * measured room responses are commonly shipped in) adds the cross-feed.  Its channel c = 2 * i + e is the response from
 * input ear i to output ear e, so the order is LL, LR, RL, RR, and an instance that names it computes
 *
 *     y_e[t] = dry * x_e[t] + wet * sum_{j=0}^{T-1} ( h_{0e}[j] * x_0[t - j] + h_{1e}[j] * x_1[t - j] )
 *
 * with everything else as for one and two channels: a four-channel IR is legal wherever an IR is named
 * (gas_conv_create, gas_conv_set_ir, gas_conv_fade_to as state A, state B or a pending target, in any combination with
 * one- and two-channel IRs, and a level-only fade).  [h_L, 0, 0, h_R] gives the bits of the two-channel [h_L, h_R].
 * dry and wet are read once per call, with no ramp, as the effect settings
 * are; the defaults dry = 0, wet = 1 suit a send bus.  The IR is the one the instance names when the call is made,
 * applied over the whole history the instance holds: gas_conv_set_ir between two calls is a hard switch at the block
 * boundary, and the history stays, because it does not depend on the IR.  Sums are f32 in a fixed order: two runs of
 * the same calls give the same bits, and an instance's output does not depend on what else a call names.
 * Out of scope: sharing one load of the two input ears between the two output ears of a true stereo instance (each
 * output ear reads both rings itself), non-uniform partitioning, gas_multi (a bus reverb belongs on the root, after the
 * gather), the host layer and godot_module/. */
#define GAS_MAX_CONVOLVERS 24 /* GAS_MAX_BUSES x GAS_MAX_CHANNELS_PER_BUS */
/* Sizes the instance pool: `convolvers` instances (<= GAS_MAX_CONVOLVERS) for IRs of up to max_ir_taps taps
 * (<= 1 048 576 = 2^20, 21.8 s at 48 kHz).  Same contract as the gas_ctx_reserve_fx_* calls: main thread, never
 * concurrently with a callback or another gas_conv_* call.  It allocates everything gas_conv_process will ever need
 * (nothing is allocated on the audio thread).  With K = ceil(max_ir_taps / cfg.frames) the bytes are
 *   per instance:  8192 K + 4096 of device memory (per ear a ring of K input spectra of 4 KiB, and the previous block);
 *   per context:   4096 + 393 216 min(32, ceil(K / 16)) + 384 cfg.frames of device memory (a twiddle table, one call's
 *                  partial sums -- two per instance and ear, for a call of 24 fading instances -- and staging) and
 *                  384 cfg.frames of pinned host memory (staging of host-memory calls);
 *   per IR (allocated by gas_conv_ir_load): 4096 channels ceil(taps / cfg.frames) of device memory, so a four-channel
 *                  IR takes four times a mono IR's.
 * (0, 0) releases everything; one of the two zero and the other not, convolvers > GAS_MAX_CONVOLVERS or max_ir_taps >
 * 2^20 is GAS_ERR_INVALID_ARGUMENT, and so is any call while an instance or an IR exists.  A HIP failure is
 * GAS_ERR_DEVICE with nothing reserved.  A context that never reserves pays nothing. */
int gas_ctx_reserve_conv(gas_ctx *ctx, uint32_t convolvers, uint32_t max_ir_taps);
/* ir = [channels][taps] f32 in host memory.  Allocates the IR's partition spectra and transforms them on the device;
 * returns when they are ready (`ir` has been consumed).  Main thread, like gas_hrtf_load.  Many instances may share
 * one IR.  channels is 1, 2 or 4 (LL, LR, RL, RR; the rule above).  GAS_ERR_INVALID_ARGUMENT: taps == 0, taps >
 * max_ir_taps, channels other than 1, 2 or 4, a value in any channel that is not finite, a NULL pointer, each with
 * nothing loaded.  GAS_ERR_UNSUPPORTED_CHAIN: nothing is reserved.  GAS_ERR_DEVICE: a HIP failure (no IR). */
int gas_conv_ir_load(gas_ctx *ctx, const float *ir /* [channels][taps] f32 */, uint32_t channels /* 1, 2 or 4 */, uint32_t taps, uint32_t *out_ir);
/* Main thread; waits for the stream.  GAS_ERR_BAD_SLOT: no such IR.  GAS_ERR_INVALID_ARGUMENT: an instance still names
 * it (nothing is freed). */
int gas_conv_ir_free(gas_ctx *ctx, uint32_t ir);
/* NEW: what gas_conv_ir_load was given, in the manner of gas_stream_get_info.  Either output may be NULL.  Touches no
 * device state.  GAS_ERR_BAD_SLOT: no such IR.  GAS_ERR_INVALID_ARGUMENT: a NULL ctx. */
int gas_conv_ir_get_info(gas_ctx *ctx, uint32_t ir, uint32_t *out_channels, uint32_t *out_taps);
/* NEW: gas_conv_ir_from_room makes an IR on the device from a box room instead of a recording.  It is declared below
 * gas_calc_early_reflections, whose gas_room and conventions it shares. */
/* Instances come from and go back to the reserved pool; these five calls allocate nothing.  Audio thread, between
 * callbacks.  An instance's ring and previous block are zeroed, in the context's stream order, when it is created and
 * by gas_conv_reset ("x[t] = 0 for all earlier t": the next call is bitwise what a fresh instance gives); levels and IR
 * survive a reset.  gas_conv_create: dry = 0, wet = 1.  GAS_ERR_UNSUPPORTED_CHAIN: nothing reserved (create).
 * GAS_ERR_OUT_OF_SLOTS: the pool is empty (create).  GAS_ERR_BAD_SLOT: an unknown instance or IR.
 * GAS_ERR_INVALID_ARGUMENT: a level that is not finite, a NULL pointer.  An error changes nothing. */
int gas_conv_create(gas_ctx *ctx, uint32_t ir, uint32_t *out_conv);
int gas_conv_destroy(gas_ctx *ctx, uint32_t conv);
int gas_conv_reset(gas_ctx *ctx, uint32_t conv); /* x[t] = 0 for all earlier t */
int gas_conv_set_ir(gas_ctx *ctx, uint32_t conv, uint32_t ir);
int gas_conv_set_levels(gas_ctx *ctx, uint32_t conv, float dry, float wet);
/* NEW: a linear fade to another impulse response and other levels over N blocks, so that a listener who walks into the
 * next room does not hear the whole reverb tail step inside one sample.  An instance has a state S = (ir, dry, wet);
 * write y^S_e[t] = dry * x_e[t] + wet * sum_j h_e[j] * x_e[t - j] for the rule above evaluated with state S over the
 * instance's one input history x (the history does not depend on the IR).  gas_conv_fade_to with N = fade_blocks >= 1
 * on an instance in state A names a target B = (ir, dry, wet): for the instance's next N gas_conv_process calls that
 * name it, frame i of the b-th such call (b = 0 .. N - 1) is
 *
 *     y[t] = (1 - s) * y^A[t] + s * y^B[t],   s = (float)(b * F + i) * (1.0f / (float)(N * F))
 *
 * with F = cfg.frames and s computed in float32 (exact for N F <= 2^21, hence the cap): the t = f * (1 / F) convention
 * of GAS_FLAG_ER_TAP_FADE stretched over N blocks.  The first frame of the fade is all A, the first frame after it all
 * B; from the (N + 1)-th call on the instance is in state B, bitwise what a hard switch to B gives over the same
 * history.  A call that does not name the instance advances neither its time nor its fade.  fade_blocks == 0 is
 * exactly gas_conv_set_ir followed by gas_conv_set_levels.  Ears and one-, two- or four-channel IRs are handled as above for
 * A and B independently.  A level-only fade (ir = the instance's current IR) is legal and computes the wet sum once.
 *  - While a fade is in progress another gas_conv_fade_to stores a pending target (the latest wins); the pending fade
 *    starts, with its own fade_blocks, at the first call after the fade in progress has ended, from state B.
 *  - gas_conv_set_ir and gas_conv_set_levels end the fade at once: the state becomes B, a pending target is dropped,
 *    then they apply as above.  gas_conv_reset zeroes the history as above and ends the fade in its final state: the
 *    pending target if there is one, else B.  gas_conv_destroy releases every IR the instance names.
 *  - A's IR, B's IR and a pending target's IR all count as named by the instance: gas_conv_ir_free on any of them is
 *    GAS_ERR_INVALID_ARGUMENT with nothing freed.  A's IR can be freed once the fade's last call has been made.
 *  - gas_conv_fade_remaining: the calls left in the fade in progress plus a pending fade's fade_blocks; 0 when the
 *    instance is settled -- the moment the old IR may be freed.
 * Both are audio-thread calls made between callbacks, like gas_conv_set_ir, and allocate nothing.  Refusals, each with
 * everything unchanged: GAS_ERR_BAD_SLOT an unknown instance or IR; GAS_ERR_INVALID_ARGUMENT a level that is not
 * finite, fade_blocks > GAS_CONV_MAX_FADE_BLOCKS, a NULL pointer.  Sums stay f32 in a fixed order: two runs of the same
 * calls give the same bits, an instance's output, fading or not, does not depend on what else a call names, and a call
 * that names no fading instance behaves as it did.  Out of scope: fades that are not linear, more than one fade
 * overlapping in time (that is what pending is for). */
#define GAS_CONV_MAX_FADE_BLOCKS 4096
int gas_conv_fade_to(gas_ctx *ctx, uint32_t conv, uint32_t ir, float dry, float wet, uint32_t fade_blocks);
int gas_conv_fade_remaining(gas_ctx *ctx, uint32_t conv, uint32_t *out_blocks);
/* out[i] = the rule over in[i] for instance convs[i], i < n; in and out are [n][frames] AudioFrames.  Audio thread.
 * GAS_MEM_DEVICE: the call only enqueues on the context's stream; `in` may be one bus of the `out` of an earlier
 * gas_process_block_buses or gas_process_block_streams_buses on the same stream (out + b * C * frames) -- the intended
 * use, and the contract gas_sidechain_set gives -- so a bus mix is convolved with no synchronisation in between.
 * Callbacks recorded or deferred before the call (GAS_FLAG_BATCHED_LAUNCH, GAS_FLAG_PIPELINED_MIX) run first.  Device
 * rows are read and written sixteen bytes at a time: in and out must be 16-byte aligned.  GAS_MEM_HOST: copy in,
 * compute, copy out; *out is complete when the call returns.  out == in (in place) is allowed; any other overlap of
 * the two, or between rows, is the caller's error.  An instance that a call does not name keeps its history and its
 * time does not advance.  n == 0 is GAS_OK.  Refusals, each with nothing changed and a host `out` zero-filled:
 * frames != cfg.frames GAS_ERR_FRAME_COUNT; an instance named twice, n > GAS_MAX_CONVOLVERS, a misaligned device
 * pointer, a bad `mem` or a NULL pointer GAS_ERR_INVALID_ARGUMENT; an unknown instance GAS_ERR_BAD_SLOT.  A HIP failure
 * is GAS_ERR_DEVICE. */
int gas_conv_process(gas_ctx *ctx, const uint32_t *convs, uint32_t n, const gas_audio_frame *in /* [n][frames] */, gas_audio_frame *out /* [n][frames] */, uint32_t frames, int mem);

/* ---- compatibility / parity path: the exact _process_frames and _mix_channel
 * signatures for one source (audio_spatializer.h:146,148), host pointers, synchronous. */
int gas_process_frames_1(gas_ctx *ctx, uint32_t slot, gas_audio_frame *out, const gas_audio_frame *src, int frame_count);
int gas_mix_channel_1(gas_ctx *ctx, uint32_t slot, int channel, gas_audio_frame *out, const gas_audio_frame *src, int frame_count);


/* ---- batched parameter generation on the device ---------------------------------
 * The arithmetic of AudioSpatializerInstance3D::calculate_spatialization (audio_spatializer_3d.cpp:277-489)
 * for n sources against n_listeners listeners in one launch: distance attenuation models (:123-151),
 * max-distance cut (:361-374), high-shelf gain (:376-388), emission cone (:378-385), stereo pan law
 * (:103-110), SPCAP surround (:56-98, :903-938), doppler pitch (:405-438), update_parameters latch
 * (:472-479).  Physics queries (Area3D override / reverb send) stay on the host.  Results are written
 * straight into the slots' device-resident parameters (as gas_params_publish would) and optionally
 * copied to out_params for the host's get_bus_map (audio_spatializer.cpp:274-324).
 * On a GAS_FLAG_HRTF_INTERPOLATE context, with hrtf_n_az and hrtf_n_el non-zero, the launch also writes each slot's
 * gas_hrtf_blend row: bilinear over the grid cell that contains (az, el).  u = az / 2pi * n_az wrapped into [0, n_az),
 * v = (el + pi/2) / pi * (n_el - 1) clamped to [0, n_el - 1]; corners (floor u, floor v), (floor u + 1 mod n_az,
 * floor v) and the same two at floor v + 1, as dir = elevation_index * n_az + azimuth_index; weights (1-fu)(1-fv),
 * fu (1-fv), (1-fu) fv, fu fv with fu, fv the fractional parts, computed in f64 and stored as f32; at n_el == 1 or v on
 * the top row the upper pair has weight 0 (and names the lower pair's cells).  hrtf_dir is written as without the flag
 * (nearest cell).  The row overrides an earlier gas_hrtf_blend_publish for the slot and is overridden by a later one;
 * it is not copied to out_params (there is no read-back of blend rows). */
typedef struct gas_spatializer3d_config { /* AudioSpatializer3D properties, audio_spatializer_3d.h:171-187 */
	int32_t attenuation_model; /* 0 inverse distance, 1 inverse square distance, 2 logarithmic, 3 disabled */
	float unit_size, max_distance, panning_strength;
	int32_t emission_angle_enabled;
	float emission_angle, emission_angle_filter_attenuation_db;
	float attenuation_filter_cutoff_hz, attenuation_filter_db;
	int32_t doppler_tracking; /* 0 = disabled */
	float doppler_speed_of_sound;
	float global_panning_strength; /* project setting audio/general/3d_panning_strength (audio_spatializer_3d.cpp:633) */
	int32_t speaker_mode; /* [ENGINE] AudioServer::SpeakerMode: 0 stereo, 1 3.1, 2 5.1, 3 7.1 */
	uint32_t hrtf_n_az, hrtf_n_el; /* NEW: azimuth x elevation grid of the loaded HRIR set; 0 = do not write hrtf_gain / hrtf_dir */
	uint32_t reserved;
} gas_spatializer3d_config;

typedef struct gas_source_pose {
	float position[3]; /* player global origin */
	float volume_db; /* AudioStreamPlayerSpatial volume_db */
	float velocity[3]; /* tracked linear velocity (used when doppler_tracking != 0) */
	float max_db;
	float forward[3]; /* player global basis column 2 (emission cone axis) */
	float pitch_scale;
} gas_source_pose;

typedef struct gas_listener { /* orthonormalized global transform of the camera / AudioListener3D */
	float basis[3][3]; /* basis[r][c]; global = basis * local + origin */
	float origin[3];
	float velocity[3];
	float pad;
} gas_listener;

#define GAS_MAX_LISTENERS 16
#define GAS_MAX_SPATIALIZER_CONFIGS 64

/* cfgs, cfg_index ([n] or NULL = config 0 for all), listeners and slots are host arrays; poses (and out_params,
 * [n] gas_params, may be NULL) are host or device pointers according to `mem`.  A slot named twice in `slots` is refused
 * with GAS_ERR_INVALID_ARGUMENT before anything is uploaded, as gas_process_block refuses it (two lanes would race on
 * the slot's row and latch).  Rows published from the host before the call (gas_params_publish[_batch]) are uploaded
 * before the launch: the launch overwrites only the fields it generates (mix_volumes, pitch_scale, linear_attenuation,
 * the cutoff, update_parameters, and hrtf_* when the config has a grid) and out_params returns the whole row, the
 * published early-reflection and shelf fields included.  The update_parameters latch (:472-479) is per slot and starts clear for a newly allocated
 * slot and after gas_source_reset.  Physics thread. */
int gas_calc_spatialization(gas_ctx *ctx, const gas_spatializer3d_config *cfgs, uint32_t n_cfgs, const uint32_t *cfg_index, const gas_source_pose *poses, const gas_listener *listeners, uint32_t n_listeners, const uint32_t *slots, uint32_t n, gas_params *out_params, int mem);

/* The same with the Area3D branches of calculate_spatialization.  The physics queries stay on the
 * host: which area a source sits in (audio_spatializer_3d.cpp:208-256) and, per listener, the closest point of the
 * area volume in that listener's space (:350-353).  The arithmetic is batched: the widened / vetoed max-distance
 * test (:364-370) and calc_reverb_vol (:154-197), max-combined over the listeners (:399-402) into the volumes the
 * reference sends to the area's reverb bus (:451-452).  Which bus that is (override / reverb bus names) is the
 * caller's bookkeeping. */
typedef struct gas_area_send {
	uint32_t using_reverb_bus; /* Area3D::is_using_reverb_bus() */
	float reverb_uniformity; /* Area3D::get_reverb_uniformity() */
	float reverb_amount; /* Area3D::get_reverb_amount() */
	uint32_t present; /* 0: the source sits in no area (other fields ignored) */
} gas_area_send;

/* areas [n], listener_area_pos [n][n_listeners][3] (may be NULL when no area has uniformity > 0) and out_reverb
 * [n][4] AudioFrames (may be NULL) are host or device pointers according to `mem`, like poses.  areas == NULL is
 * gas_calc_spatialization. */
int gas_calc_spatialization_areas(gas_ctx *ctx, const gas_spatializer3d_config *cfgs, uint32_t n_cfgs, const uint32_t *cfg_index, const gas_source_pose *poses, const gas_listener *listeners, uint32_t n_listeners, const uint32_t *slots, uint32_t n, const gas_area_send *areas, const float *listener_area_pos, gas_params *out_params, gas_audio_frame *out_reverb, int mem);

/* ---- the producer of GAS_FX_EARLY_REFLECTIONS' parameters -------------------------------------------
 * NEW (the effect has no counterpart in the engine, and neither has this).  n sources and one listener inside
 * axis-aligned box rooms: the image sources up to second order, the eight strongest of them as er_gain / er_delay,
 * in one launch per physics tick.
 *
 * The rule, in float32 in this order, no fused multiply-adds.  M = er_ring_frames - frames, rate = the context's
 * mix_rate, h = half_extent, c = speed_of_sound.
 *  1. s = basis^T (position - origin), l = basis^T (listener->origin - origin): both in the room's frame.
 *  2. room_index[i] == GAS_ROOM_NONE, or any |s_a| > h_a, or any |l_a| > h_a: all eight taps are (gain 0, delay 1).
 *  3. d0 = |s - l|: sqrtf of the sum of the squares in x, y, z order.
 *  4. The candidates are the 24 integer triples m with 1 <= |m_x| + |m_y| + |m_z| <= 2, numbered in ascending order
 *     of (|m|_1, m_x, m_y, m_z): (-1,0,0), (0,-1,0), (0,0,-1), (0,0,1), (0,1,0), (1,0,0), (-2,0,0), (-1,-1,0), ...
 *  5. img_a = 2 m_a h_a + (m_a odd ? -s_a : s_a); dist = |img - l|.  R starts at 1 and, in axis order x, y, z, is
 *     multiplied p_a times by the +a wall's reflectance, then q_a times by the -a wall's: p_a = ceil(m_a / 2),
 *     q_a = floor(m_a / 2) for m_a > 0, swapped for m_a < 0.  g = ((level R) d0) / dist -- the reflection relative to
 *     the direct sound under 1/r, so g <= level.  fr = ((dist - d0) / c) rate; delay_raw = rintf(fr), ties to even.
 *  6. g becomes 0 when |m|_1 > max_order, when !(dist > 0), when g is not finite, or when delay_raw > M: the ring does
 *     not reach that far, and the effect's own clamp would put the echo at the wrong time.  delay = max(delay_raw, 1).
 *  7. Tap k takes the candidate of rank k, by g descending, ties to the lower candidate number.  A tap whose
 *     candidate has g == 0 is written as (0, 1).
 * Not modelled: a direction per reflection, smoothing of the taps between callbacks (the effect switches gains and
 * delays at block boundaries), rooms that are no boxes, occlusion. */
#define GAS_MAX_ROOMS 64
#define GAS_ROOM_NONE 0xffffffffu
typedef struct gas_room { /* NEW; 96 bytes */
	float basis[3][3]; /* global = basis * local + origin, orthonormal (as gas_listener) */
	float origin[3]; /* centre of the box */
	float half_extent[3]; /* > 0 */
	float reflectance[6]; /* amplitude factor per wall, 0 .. 1: -x, +x, -y, +y, -z, +z */
	float speed_of_sound; /* > 0, metres per second */
	float level; /* >= 0, linear, on every reflection */
	uint32_t max_order; /* 1 or 2 */
} gas_room;
typedef struct gas_er_taps {
	float gain[GAS_ER_TAPS];
	uint32_t delay[GAS_ER_TAPS];
} gas_er_taps;

/* rooms [n_rooms], 1 <= n_rooms <= GAS_MAX_ROOMS, room_index ([n] or NULL = room 0 for all; GAS_ROOM_NONE = the source
 * sits in no room), listener (one; only its origin is read) and slots ([n] or NULL) are host arrays; poses ([n]; only
 * position is read) and out_taps ([n], may be NULL) are host or device pointers according to `mem`.
 * slots != NULL: the taps go into the slots' rows of the parameter table, the rows gas_calc_spatialization writes.
 * Recorded or deferred batched callbacks run first, and rows published from the host before the call are uploaded
 * before the launch, which overwrites er_gain and er_delay and nothing else.  It does not make a slot "have
 * parameters": a slot that never got a whole row is still refused by gas_process_block with GAS_ERR_NO_PARAMS.  A later
 * gas_params_publish[_batch] of the slot replaces the whole row, these fields included, as it replaces
 * gas_calc_spatialization's -- so within a tick: publish, then gas_calc_spatialization, then this call.
 * slots == NULL: a pure generator.  Nothing in the context changes and out_taps is required.  (The road for gas_host_*
 * users, whose rows are published whole on the audio thread: merge the taps into the POD and publish that.)
 * out_taps, when given, holds exactly what was generated, in either mode.
 * GAS_ERR_INVALID_ARGUMENT, with nothing written: a NULL ctx / rooms / poses / listener; slots and out_taps both NULL;
 * a bad mem; n_rooms 0 or > GAS_MAX_ROOMS; n > max_sources; a context with er_ring_frames == 0; a room_index[i] that
 * is neither < n_rooms nor GAS_ROOM_NONE; a slot named twice; a room whose half_extent or speed_of_sound is not
 * positive and finite, whose level is negative or not finite, with a reflectance outside [0, 1] or a max_order other
 * than 1 or 2.  GAS_ERR_BAD_SLOT: a slot that is not in use.  n == 0 is GAS_OK.
 * Physics thread: it shares gas_calc_spatialization's lock and staging buffers. */
int gas_calc_early_reflections(gas_ctx *ctx, const gas_room *rooms, uint32_t n_rooms, const uint32_t *room_index, const gas_source_pose *poses, const gas_listener *listener, const uint32_t *slots, uint32_t n, gas_er_taps *out_taps, int mem);

/* ---- a convolver's impulse response from a box room (it belongs to the gas_conv_* calls above and stands here because
 * it takes a gas_room and a gas_listener by value) ------------------------------------------------------------------
 * NEW.  The image-source lattice of Allen & Berkley that gas_calc_early_reflections cuts off at order 2, summed into an
 * impulse response of `taps` taps on the device and handed straight to the transform gas_conv_ir_load uses.  Levels and
 * times are gas_calc_early_reflections': tap 0 is the arrival of the direct sound and a reflection's gain is relative to
 * it, so the ER taps of the sources (orders 1 - 2) and a generated tail with min_order = 3 on the send bus add up to one
 * room response with nothing counted twice.
 *
 * The rule.  Inputs are float32 and are widened to float64; everything up to the final conversion is float64 with no
 * fused multiply-adds.  h = half_extent, c = speed_of_sound, rate = the context's mix_rate, B = room.basis.
 *  1. s = B^T (source - origin), l = B^T (listener.origin - origin), r = B^T (listener.basis column 0); d0 = |s - l|.
 *     Receivers: one channel e_0 = l; two channels e_0 = l - (ear_spacing / 2) r, e_1 = l + (ear_spacing / 2) r.
 *  2. reach = c taps / rate + d0 + (channels == 2 ? ear_spacing / 2 : 0); N_a = floor(reach / (2 h_a)) + 1, clamped to
 *     max_order when max_order != 0.  The candidates are the integer triples m with |m_a| <= N_a and min_order <= |m|_1
 *     (and |m|_1 <= max_order when it is not 0).  No image outside this box can reach tap taps - 1.
 *  3. Per image, steps 5 and 6 of gas_calc_early_reflections: img_a = 2 m_a h_a + (m_a odd ? -s_a : s_a); R is the
 *     product over the axes of the +a wall's reflectance p_a times and the -a wall's q_a times, p_a = ceil(m_a / 2),
 *     q_a = floor(m_a / 2) for m_a > 0, swapped for m_a < 0; each axis' factor is a running product over |m_a| = 1, 2, ...
 *     and R = (R_x R_y) R_z.  m = 0 is the direct sound, R = 1.
 *  4. Per receiver e: dist = |img - e_e|; v = R d0 / max(dist, d0), so v <= 1 (the clamp only ever bites for an ear that
 *     is nearer than the head's centre); pos = ((dist - d0) / c) rate, which is gas_calc_early_reflections' fr;
 *     k = floor(pos), f = pos - k; tap k receives v (1 - f) and tap k + 1 receives v f.  A tap index outside [0, taps) is
 *     dropped on its own: an image with k = -1 still feeds tap 0, so the rule is continuous in every input.
 *  5. Each of the two shares is quantised to q = llrint(share 2^32) and summed into one int64 per channel and tap.
 *     Integer sums are associative: any order of arrival gives the same bits, and two runs of the same call do.  At most
 *     2^28 candidates with v <= 1 keep a sum below 2^61.
 *  6. h_e[k] = (float)((double)level (double)acc_e[k] 2^-32).
 *
 * out_ir != NULL: the result becomes an IR like any gas_conv_ir_load gives -- usable in gas_conv_create, gas_conv_set_ir
 * and gas_conv_fade_to, freed by gas_conv_ir_free, reported by gas_conv_ir_get_info.  The taps never visit the host on
 * this path.  out_taps != NULL: the float32 taps are copied back, [channels][taps].  With out_ir == NULL the call is a
 * pure generator: it needs no reserved pool and touches no context state, like gas_calc_early_reflections with
 * slots == NULL.  Main thread, the contract of gas_conv_ir_load: deferred and recorded callbacks are flushed first (when
 * an IR is loaded) and the call returns when the IR is ready.  The temporaries (8 channels taps bytes of sums,
 * 4 channels taps of taps, the reflectance tables) are freed on every way out.  While gas_profile_enable is on, the
 * generator's launches (zeroing, sums, scaling; not the transform) are bracketed and counted by gas_profile_read as a
 * callback's dominant launch is -- the one way in which a profiled pure generator touches the context.
 * Refusals, each with nothing loaded and nothing written.  GAS_ERR_INVALID_ARGUMENT: a NULL ctx or desc; out_taps and
 * out_ir both NULL; channels other than 1 or 2; taps == 0; taps > max_ir_taps of the reserve when out_ir != NULL, or
 * taps > 2^20 for the pure generator; a room that gas_calc_early_reflections would refuse (room.max_order is not read);
 * min_order > max_order when max_order != 0; an ear_spacing that is negative or not finite; a coordinate (room basis or
 * origin, source, listener basis or origin) that is not finite; |s_a| > h_a or |l_a| > h_a on any axis; d0 < 1e-3;
 * (2 N_x + 1)(2 N_y + 1)(2 N_z + 1) > 2^28 -- the remedy is a shorter IR or a max_order; the check is made from step 2
 * before anything is launched.  GAS_ERR_UNSUPPORTED_CHAIN: out_ir != NULL with nothing reserved.  GAS_ERR_DEVICE: a HIP
 * failure, with no IR loaded.
 * Out of scope: frequency-dependent absorption, air absorption, jitter against flutter echoes, a direction-dependent
 * (HRTF) receiver, four-channel results, rooms that are not boxes, the host layer, godot_module/ and gas_multi.
 * (The HRTF receiver is a call of its own, gas_conv_ir_from_room_hrtf, and so are rooms that are not boxes,
 * gas_conv_ir_from_planes; both are declared below this one.) */
typedef struct gas_room_ir { /* NEW; 184 bytes */
	gas_room room; /* as for gas_calc_early_reflections; room.max_order is NOT read here */
	float source[3]; /* global position of the emitter that stands for the bus */
	gas_listener listener; /* origin and basis are read (local +x = right ear side); velocity is not */
	float ear_spacing; /* metres between the two receivers of a two-channel IR, >= 0; ignored for one channel */
	uint32_t min_order; /* images with |m|_1 < min_order are left out: 3 = "behind ER at max_order 2", 1 = no direct sound */
	uint32_t max_order; /* images with |m|_1 > max_order are left out; 0 = no limit but the IR's length */
} gas_room_ir;
int gas_conv_ir_from_room(gas_ctx *ctx, const gas_room_ir *desc, uint32_t channels /* 1 or 2 */, uint32_t taps, float *out_taps /* host [channels][taps], may be NULL */, uint32_t *out_ir /* may be NULL */);

/* NEW: gas_conv_ir_from_planes -- the image-source method for a room that is no box: up to GAS_ROOM_MAX_PLANES
 * half-spaces, each with a reflectance.  An attic, a corridor with a slanted wall, a hexagonal hall; the planes need not
 * close a room, so a lone ground plane or two facing walls are rooms as well.  Levels and times are
 * gas_conv_ir_from_room's: tap 0 is the arrival of the direct sound and a reflection's gain is relative to it.  The method
 * walks plane sequences, P (P - 1)^(K - 1) of them at order K, so it is one for low orders -- the image part in front of
 * a diffuse tail -- and max_order is required.
 *
 * The rule.  Inputs are float32 and are widened to float64; everything up to the final conversion is float64 with no
 * fused multiply-adds.  dot(n, x) = (n_x x_x + n_y x_y) + n_z x_z.  P = n_planes, c = speed_of_sound, rate = the context's
 * mix_rate.
 *  1. Geometry.  n_j = the widened normal divided, per component, by its length sqrt((x x + y y) + z z); d_j = offset.
 *     s = source, l = listener.origin, r = listener.basis column 0.  d0 = |s - l| = sqrt((dx dx + dy dy) + dz dz).
 *     Receivers: one channel e_0 = l; two channels e_0 = l - (ear_spacing / 2) r, e_1 = l + (ear_spacing / 2) r.
 *  2. Candidates.  The plane sequences q_1 .. q_K with q_i != q_{i+1}, for max(min_order, 1) <= K <= max_order:
 *     P (P - 1)^(K - 1) per order (for P = 1 only K = 1).  For min_order == 0 there is also the direct sound: image = s,
 *     R = 1, nothing to validate.
 *  3. Images.  I_0 = s.  For i = 1 .. K: t = dot(n_{q_i}, I_{i-1}) - d_{q_i}; the sequence is void unless t > 0;
 *     I_i = I_{i-1} - (2 t) n_{q_i}, per component.  R is the running product of the planes' reflectances in sequence
 *     order.
 *  4. Validity, per receiver e.  p = e.  For i = K down to 1: a = dot(n_{q_i}, p) - d_{q_i} and
 *     b = dot(n_{q_i}, I_i) - d_{q_i}; the path is invalid unless a > 0; u = a / (a - b); hit = p + u (I_i - p), per
 *     component; the path is invalid unless dot(n_j, hit) - d_j >= 0 for every j != q_i; then p = hit.  The test is
 *     closed: a path through an exact edge of the room may pass for both orders of the two planes and count twice.
 *  5. Taps, for a valid path: dist = |I_K - e|, as d0 is computed.  Then steps 4 to 6 of gas_conv_ir_from_room, unchanged:
 *     v = R d0 / max(dist, d0); pos = ((dist - d0) / c) rate; k = floor(pos), f = pos - k; tap k receives v (1 - f) and
 *     tap k + 1 receives v f, a tap index outside [0, taps) dropped on its own; each share is quantised to
 *     llrint(share 2^32) and summed into one int64 per channel and tap, so no order of arrival changes a bit; and
 *     h_e[k] = (float)((double)level (double)acc_e[k] 2^-32).
 *
 * Consequences.  A box given as its six planes has the images of gas_conv_ir_from_room with that max_order (same points,
 * reached by another road of float64 operations: the two agree within the last float32 bit, not by contract to the bit).
 * Swapping source and listener gives the same one-channel taps within that.  Two calls give the same bits.
 *
 * out_ir, out_taps, the pure generator (out_ir == NULL: no reserve needed, no context state touched), the main thread,
 * the flush of deferred and recorded callbacks when an IR is loaded, the temporaries (8 channels taps bytes of sums,
 * 4 channels taps of taps; the planes travel as a kernel argument) freed on every way out, and the profiling bracket
 * (zeroing, sums, scaling; not the transform) are as for gas_conv_ir_from_room.
 * Refusals, each with nothing loaded and nothing written.  GAS_ERR_INVALID_ARGUMENT: a NULL ctx or desc; out_taps and
 * out_ir both NULL; channels other than 1 or 2; taps == 0; taps > max_ir_taps of the reserve when out_ir != NULL, or
 * taps > 2^20 for the pure generator; n_planes 0 or above GAS_ROOM_MAX_PLANES; max_order 0 or above
 * GAS_ROOM_PLANES_MAX_ORDER; min_order > max_order; a value that is read and is not finite (planes beyond n_planes and
 * listener fields other than origin and basis column 0 are not read); a normal whose length is outside [0.999, 1.001]; a
 * reflectance outside [0, 1]; a speed_of_sound that is not positive; a negative level or ear_spacing (ear_spacing is
 * checked for one channel too); the source or a receiver with dot(n_j, x) - d_j <= 0 for some j; d0 < 1e-3; more than
 * 2^28 candidate sequences over all orders (the direct sound is not counted) -- computed from P and the orders before
 * anything is launched.  GAS_ERR_UNSUPPORTED_CHAIN: out_ir != NULL with nothing reserved.  GAS_ERR_DEVICE: a HIP failure,
 * with no IR loaded.
 * Out of scope: non-convex rooms and occlusion (every plane bounds the whole room); per-band reflectances and air
 * absorption for planes; an HRTF receiver (the spreading phase of gas_conv_ir_from_room_hrtf's kernel would serve it); a
 * diffuse tail, which needs the room's volume and face areas from the planes -- until it exists a caller adds the
 * out_taps of a box's gas_conv_ir_from_room_diffuse on the host; early-reflection taps from planes; a per-order frontier
 * with compaction in place of the enumeration of every sequence; the host layer, godot_module/ and gas_multi. */
#define GAS_ROOM_MAX_PLANES 16
#define GAS_ROOM_PLANES_MAX_ORDER 8
typedef struct gas_room_plane { /* NEW; 20 bytes */
	float normal[3]; /* unit length, pointing into the room */
	float offset; /* inside: dot(normal, x) - offset > 0 */
	float reflectance; /* amplitude factor, 0 .. 1 */
} gas_room_plane;
typedef struct gas_room_planes { /* NEW; 420 bytes */
	gas_room_plane planes[GAS_ROOM_MAX_PLANES]; /* inside: dot(normal, x) - offset > 0, global coordinates, inward unit normals */
	uint32_t n_planes; /* 1 .. GAS_ROOM_MAX_PLANES; the planes need not bound a closed room */
	float speed_of_sound; /* > 0 */
	float level; /* >= 0, as gas_room.level */
	float source[3]; /* global position of the emitter that stands for the bus */
	gas_listener listener; /* origin and basis column 0 are read, as in gas_room_ir */
	float ear_spacing; /* as in gas_room_ir */
	uint32_t min_order; /* 0 includes the direct sound */
	uint32_t max_order; /* 1 .. GAS_ROOM_PLANES_MAX_ORDER, required */
} gas_room_planes;
int gas_conv_ir_from_planes(gas_ctx *ctx, const gas_room_planes *desc, uint32_t channels /* 1 or 2 */, uint32_t taps, float *out_taps /* host [channels][taps], may be NULL */, uint32_t *out_ir /* may be NULL */);

/* NEW: gas_conv_ir_from_room_hrtf -- the same box room heard binaurally: every image arrives through the HRIR pair of its
 * direction, so the tail carries the pinna and head cues the dry GAS_FX_HRTF sources have, from the same HRIR set.  The
 * result always has two channels: ear 0 is left, ear 1 is right.  `hrir` is the gridded set the caller gave gas_hrtf_load
 * (or received as out_hrir from gas_hrtf_load_positions), float32 [n_az * n_el][2 ears][hrir_taps], with the direction
 * convention of hrtf_dir = elevation_index * n_az + azimuth_index.  It is passed in because the context keeps only
 * spectra, and so that the pure generator (out_ir == NULL) stays free of context state.  desc->ear_spacing is neither
 * read nor validated.  ER taps on the sources (orders 1 - 2) plus this tail with min_order = 3 on the send bus form one
 * room, heard through the HRIR set of the dry sound.
 *
 * The rule.  Inputs are float32 and are widened to float64; everything up to the final conversion is float64 with no
 * fused multiply-adds.
 *  1. Steps 1 - 3 of gas_conv_ir_from_room with channels = 1: one receiver e_0 = l, reach without the ear term; the
 *     candidate box, the order masks, R from the running products and the refusal above 2^28 cells are the same.
 *  2. Per image, step 4 with the receiver l: dist = |img - l|; v = R d0 / max(dist, d0); pos = ((dist - d0) / c) rate;
 *     k = floor(pos), f = pos - k; a0 = v (1 - f), a1 = v f.  A reflected path is never shorter than the direct one, so
 *     k >= 0; an image with k >= taps contributes nothing.
 *  3. Direction of arrival in the listener's frame.  w = img - l (room's frame), B = room.basis, L = listener.basis:
 *     g_a = B[a][0] w_0 + B[a][1] w_1 + B[a][2] w_2;  p_a = L[0][a] g_0 + L[1][a] g_1 + L[2][a] g_2, each sum in that
 *     order.  The cell is chosen as gas_calc_spatialization chooses hrtf_dir: az = atan2(p_x, -p_z),
 *     flat = sqrt(p_x p_x + p_z p_z), el = atan2(p_y, flat); ai = llround(az / 2pi n_az) wrapped into [0, n_az);
 *     ei = n_el > 1 ? llround((el + pi/2) / pi (n_el - 1)) : 0, clamped to [0, n_el - 1]; dir = ei n_az + ai.  For m = 0
 *     this is the cell gas_calc_spatialization writes as the source's hrtf_dir.
 *  4. For ear e and j = 0 .. hrir_taps, with H = hrir widened and H[dir][e][-1] = H[dir][e][hrir_taps] = 0:
 *     g_j = a0 H[dir][e][j] + a1 H[dir][e][j - 1] (two products, one sum); q = llrint(g_j 2^32), signed;
 *     acc_e[k + j] += q when k + j < taps -- each tap is dropped on its own.  This is the HRIR shifted by the fractional
 *     delay the one-channel rule uses.
 *  5. h_e[t] = (float)((double)level (double)acc_e[t] 2^-32).
 * Overflow: an hrir value above 4 in magnitude is refused, so a tap receives at most 4 v <= 4 per image and at most 2^28
 * images keep the int64 sums below 2^62.
 * Consequences.  With the set H[d][e][0] = 1 and everything else 0, both channels are bitwise the one-channel
 * gas_conv_ir_from_room of the same descriptor (a0 1 + a1 0 is a0 exactly).  Orders [0, 2] plus [3, inf) equal [0, inf)
 * exactly in the integer sums.  Two runs of one call give the same bits.
 *
 * out_ir, out_taps ([2][taps]), threading, the flushing of deferred callbacks, the gas_profile_enable bracket and the
 * freeing of the temporaries (8 2 taps bytes of sums, 4 2 taps of taps, the reflectance tables, the set) on every way out
 * are as for gas_conv_ir_from_room.
 * Refusals, each with nothing loaded and nothing written.  GAS_ERR_INVALID_ARGUMENT: everything gas_conv_ir_from_room
 * refuses with channels = 1, except the ear_spacing checks; a NULL hrir; n_az == 0, n_el == 0 or n_az n_el > 65 536;
 * hrir_taps == 0 or hrir_taps > GAS_HRTF_TAPS; an hrir value that is not finite or above 4 in magnitude.
 * GAS_ERR_UNSUPPORTED_CHAIN: out_ir != NULL with nothing reserved.  GAS_ERR_DEVICE: a HIP failure, with no IR loaded.
 * Out of scope: bilinear blending of the four surrounding cells (nearest cell only, as hrtf_dir), four-channel results,
 * a per-reflection direction for GAS_FX_EARLY_REFLECTIONS, frequency-dependent absorption and air absorption, the
 * shell-per-workgroup shape, the host layer, godot_module/ and gas_multi. */
int gas_conv_ir_from_room_hrtf(gas_ctx *ctx, const gas_room_ir *desc, const float *hrir /* host [n_az * n_el][2 ears][hrir_taps] f32 */, uint32_t n_az, uint32_t n_el, uint32_t hrir_taps /* 1 .. GAS_HRTF_TAPS */, uint32_t taps, float *out_taps /* host [2][taps], may be NULL */, uint32_t *out_ir /* may be NULL */);

/* NEW: gas_conv_ir_from_room_bands and gas_conv_ir_from_room_hrtf_bands -- the two calls above with walls that absorb
 * differently per frequency band and with air that absorbs over distance.  With one broadband reflectance per wall every
 * image arrives with a flat spectrum and all frequencies decay at one rate; here the spectrum is split into B bands by
 * linear-phase filters, each band has its own six reflectances and its own loss per metre, and the bands are summed.
 * desc->room.reflectance is validated as before but not used: bands->reflectance[b] takes its place.
 *
 * The rule.  Inputs are float32 and are widened to float64; everything up to the final conversion is float64.
 *  1. Band sums.  For each band b < B = n_bands, acc_b[e][k] are the int64 sums of steps 1 - 5 of gas_conv_ir_from_room
 *     with room.reflectance := bands.reflectance[b] (for the _hrtf call: steps 1 - 4 of gas_conv_ir_from_room_hrtf).  The
 *     candidate box, the order masks and the refusal above 2^28 cells do not depend on a reflectance and are the same for
 *     every band.
 *  2. Air.  c = speed_of_sound, rate = mix_rate:  lambda_b = (ln 10 / 20) air_db_per_m[b] c / rate, left to right;
 *     g_b[k] = exp(-(lambda_b k));  u_b[e][k] = ((double)acc_b[e][k] 2^-32) g_b[k].  Tap k lies k c / rate metres beyond
 *     the direct path, so this is attenuation over distance written as a function of time.  At air_db_per_m[b] == 0,
 *     g is exactly 1.
 *  3. Band filters, L = filter_taps, D = (L - 1) / 2, built on the host:
 *     w[j] = 0.42 - 0.5 cos(2 pi j / (L - 1)) + 0.08 cos(4 pi j / (L - 1));  for crossover i, nu = crossover_hz[i] / rate,
 *     s_i[j] = w[j] (j == D ? 2 nu : sin(2 pi nu (j - D)) / (pi (j - D)));  lp_i = s_i / sum_j s_i[j], the sum taken in
 *     ascending j.  F_0 = lp_0;  F_b = lp_b - lp_(b-1) for 0 < b < B - 1;  F_(B-1) = delta_D - lp_(B-2).  For B == 1,
 *     F_0 = delta_D with L = 1, D = 0 (filter_taps is not read).  The filters sum to delta_D by construction.
 *  4. Combine.  y[e][t] = sum_b sum_(j<L) F_b[j] u_b[e][t + D - j]; a term whose index t + D - j falls outside [0, taps)
 *     is dropped.  The D samples of delay of the linear-phase filters are taken back out: tap 0 stays the arrival of the
 *     direct sound.  The order of summation is fixed (bands ascending, within a band j descending, one running sum per
 *     tap, each product fused into the sum) and nothing in this step is atomic.
 *  5. Scale.  h[e][t] = (float)((double)level y[e][t]).
 * Consequences.  B == 1 with air_db_per_m[0] == 0 is bitwise gas_conv_ir_from_room of a descriptor whose room.reflectance
 * is reflectance[0] (a product with 1 and a power of two are exact); the _hrtf call likewise.  With every band's
 * reflectances equal and no air the result equals the plain call's within float32's last rounding (4e-9 to 7e-9 relative
 * RMS in the float64 reference).  The direct sound of a min_order = 0 result arrives at tap 0 as exactly `level`, whatever
 * the bands and the air: it has R = 1 in every band, g_b[0] = 1, and the filters sum to delta_D (with every wall dead
 * tap 0 is `level` to the bit and the other taps hold what the float64 sum of the filters leaves, below 1e-15; with
 * live walls whose bands differ, reflections within D taps of tap 0 reach it through the band filters as they reach
 * every tap near them).  Two runs of one call give the same bits.
 *
 * out_ir, out_taps, threading, the flushing of deferred callbacks, the gas_profile_enable bracket (B zeroings, B sums,
 * B scalings and the combine) and the freeing of the temporaries (B times the plain call's sums and tables, the filter
 * table of B L float64) on every way out are as for the plain call of the same name.
 * Refusals, each with nothing loaded and nothing written.  GAS_ERR_INVALID_ARGUMENT: everything the plain call of the
 * same name refuses; a NULL bands; n_bands == 0 or n_bands > GAS_ROOM_MAX_BANDS; for B > 1 a filter_taps that is even,
 * below 3 or above GAS_ROOM_BAND_FILTER_MAX_TAPS; a crossover among the B - 1 read that is not finite, not positive,
 * not below rate / 2 or not strictly above its predecessor; a reflectance in the B rows read that is outside [0, 1] (a
 * NaN is); an air_db_per_m among the B read that is negative or not finite; reserved != 0.  Entries beyond B (beyond
 * B - 1 for crossovers) are neither read nor checked.  GAS_ERR_UNSUPPORTED_CHAIN and GAS_ERR_DEVICE: as for the plain
 * calls.
 * Out of scope: jitter against flutter echoes (a diffuse late tail is a call of its own, gas_conv_ir_from_room_diffuse,
 * declared below), minimum-phase band filters, a level per band, rooms that are not boxes
 * (gas_conv_ir_from_planes, above, makes their image part, broadband), bands for gas_calc_early_reflections' taps, the host layer, godot_module/ and gas_multi. */
#define GAS_ROOM_MAX_BANDS 8
#define GAS_ROOM_BAND_FILTER_MAX_TAPS 4095
typedef struct gas_room_bands { /* NEW; 264 bytes */
	uint32_t n_bands; /* B: 1 .. GAS_ROOM_MAX_BANDS */
	uint32_t filter_taps; /* L: odd, 3 .. GAS_ROOM_BAND_FILTER_MAX_TAPS; not read when B == 1 */
	float crossover_hz[GAS_ROOM_MAX_BANDS - 1]; /* B - 1 read: strictly ascending, 0 < c < mix_rate / 2 */
	float reflectance[GAS_ROOM_MAX_BANDS][6]; /* per band, wall order of gas_room; 0 .. 1; B rows read */
	float air_db_per_m[GAS_ROOM_MAX_BANDS]; /* per band, >= 0, finite: dB lost per metre of path beyond the direct path */
	uint32_t reserved; /* 0 */
} gas_room_bands;
int gas_conv_ir_from_room_bands(gas_ctx *ctx, const gas_room_ir *desc, const gas_room_bands *bands, uint32_t channels /* 1 or 2 */, uint32_t taps, float *out_taps /* host [channels][taps], may be NULL */, uint32_t *out_ir /* may be NULL */);
int gas_conv_ir_from_room_hrtf_bands(gas_ctx *ctx, const gas_room_ir *desc, const gas_room_bands *bands, const float *hrir /* host [n_az * n_el][2 ears][hrir_taps] f32 */, uint32_t n_az, uint32_t n_el, uint32_t hrir_taps /* 1 .. GAS_HRTF_TAPS */, uint32_t taps, float *out_taps /* host [2][taps], may be NULL */, uint32_t *out_ir /* may be NULL */);

/* NEW: gas_conv_ir_from_room_diffuse and gas_conv_ir_from_room_hrtf_diffuse -- the two *_bands calls above with a diffuse
 * late tail behind the image sources.  A box with mirror walls is not a diffuse room: out to the last tap the image
 * lattice keeps the flutter and the sweeping echoes the method is known for, its late energy decays more slowly than a
 * room's (paths along the least absorbing axis survive), and its cost grows with the cube of the response's length.
 * Here the images are kept up to a mixing time; from there the response cross-fades into shaped noise whose decay per
 * band follows the room's mean absorption by Eyring's formula, and the lattice is walked for the specular part alone.
 * `bands` is required; a broadband room is n_bands = 1.  This is NEW behaviour with no engine counterpart.
 *
 * The rule.  Inputs are float32 and are widened to float64; everything up to the final conversion is float64, left to
 * right, with no fused multiply-adds except where the *_bands rule allows them.  rate = mix_rate, c = speed_of_sound,
 * h = half_extent, d0 as in step 1 of gas_conv_ir_from_room, B = n_bands.
 *  1. Fade marks.  K0 = min(taps, llrint(min(mix_time_s rate, 2^31)));  K1 = min(taps, K0 + llrint(min(fade_s rate,
 *     2^31)));  Kf = K1 - K0.  For tap k: x = k < K0 ? 0 : (k >= K1 ? 1 : (k - K0) / Kf);  ws[k] = sqrt(1 - x),
 *     wd[k] = sqrt(x).  The two are power-complementary, and sqrt is correctly rounded on every side.
 *  2. Specular sums.  acc_b[e][k] for k < K1 are the int64 band sums of step 1 of the *_bands rule (for the _hrtf call:
 *     those of gas_conv_ir_from_room_hrtf_bands); order masks, min_order and max_order apply as there.  Taps k >= K1 take
 *     nothing specular.  By step 2 of gas_conv_ir_from_room no image outside the candidate box for K1 taps reaches a tap
 *     below K1, so the lattice passes run as for an IR of K1 taps, and the refusal above 2^28 cells is evaluated for K1
 *     taps, not for `taps`.  With K1 == 0 there is no lattice pass and no cell check.
 *  3. Decay per band.  V = 8 h_x h_y h_z;  A_x = 4 h_y h_z, A_y = 4 h_x h_z, A_z = 4 h_x h_y;  S = 2 (A_x + A_y + A_z).
 *     With R = bands.reflectance[b]:  rho_b = (A_x (R[0] R[0] + R[1] R[1]) + A_y (R[2] R[2] + R[3] R[3]) +
 *     A_z (R[4] R[4] + R[5] R[5])) / S, the walls' mean energy reflectance;  mu_b = -ln(rho_b) S / (4 V), the energy lost
 *     per metre (Eyring).  rho_b == 0 makes the band's diffuse part 0.
 *     s0 = gain sqrt(((4 pi c) (d0 d0)) / (V rate)): the echo density 4 pi r^2 (c / rate) / V times (d0 / r)^2, so the
 *     level is relative to the direct sound as every image's v is.  r_k = d0 + c k / rate.  Air is not applied here:
 *     step 2 of the *_bands rule applies g_b[k] to whatever the sums hold, the diffuse part included.
 *  4. Noise, one stream per ear, shared by all bands, so that the band filters still sum to a delta over it.  In 64-bit
 *     unsigned arithmetic mod 2^64:  z = (seed << 32) | (e << 24) | k;  z += 0x9E3779B97F4A7C15;
 *     z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) 0x94D049BB133111EB;  z ^= z >> 31;
 *     u_i = (z >> 16 i) & 0xffff.  xi[e][k] = (2 (u_0 + u_1 + u_2) - 196605) / sqrt(65536^2 - 1): unit variance, odd
 *     integer numerators.  f[e][k] = (u_3 + 0.5) / 65536.
 *     Check vectors (seed, e, k) -> z, numerator:  (1, 0, 0) -> 0xc42c5a1aa3820138, -66133;
 *     (1, 0, 1) -> 0x204391a6fd59956f, 84191;  (0, 1, 5) -> 0x554b78b0c52407ed, -29819;
 *     (0xffffffff, 1, 2^20 - 1) -> 0x5e823beaa35dc300, 17553.
 *  5. Arrivals, split as images are.  a_b[e][k] = (s0 exp(-(mu_b r_k) / 2)) xi[e][k];
 *     d_b[e][k] = a_b[e][k] (1 - f[e][k]) + a_b[e][k - 1] f[e][k - 1], the second term absent at k = 0.  The diffuse part
 *     so has the two-tap interpolation spectrum of the image taps and the same 2/3 of an arrival's energy per tap.
 *  6. Mix.  acc'_b[e][k] = llrint(ws[k] (double)acc_b[e][k]) + llrint((wd[k] d_b[e][k]) 2^32); the first term is 0 for
 *     k >= K1, and for k < K0 the result is acc_b[e][k] exactly.
 *  7. Finish.  Steps 2 - 5 of the *_bands rule (air, band filters, combine, scale by level) over acc' at the full `taps`.
 * Overflow: s0 <= 1024 is required, so |llrint((wd d) 2^32)| < 2^44 and the int64 sums stay below 2^62.
 * Consequences (D = the band filters' delay, 0 for B == 1).  With K0 == taps the result is bitwise the *_bands call of the
 * same name.  With gain == 0 every tap t >= K1 + D is exactly 0.  Taps t < K0 - D are bitwise the *_bands call's whatever
 * the tail.  Two runs give the same bits; another seed gives other taps from K0 on.  Through unit-impulse HRIRs the
 * specular part of the _hrtf call is the one-channel sums in both ears, as for the calls above; its diffuse parts differ
 * per ear.  ER taps on the sources plus a min_order = 3 tail keep working: the diffuse part starts at K0 whatever the
 * orders are.
 * Known limits.  The level at the hand-over is theory, not a fit: `gain` is the trim.  The coherent low-frequency
 * build-up of an image part whose reflectances are all positive is not reproduced by zero-mean noise.  The diffuse parts
 * of the two ears are uncorrelated at all frequencies, and the _hrtf call's diffuse part is not coloured by the set.
 *
 * out_ir, out_taps, the pure generator, threading, the flushing of deferred callbacks, the gas_profile_enable bracket
 * (the *_bands call's launches for K1 taps, the tail kernel and the combine) and the freeing of the temporaries (those
 * of the *_bands call, its sums once for K1 taps and once for `taps`) on every way out are as for the *_bands call of the
 * same name.  gas_abi_version() is unchanged.
 * Refusals, each with nothing loaded and nothing written.  GAS_ERR_INVALID_ARGUMENT: everything the *_bands call of the
 * same name refuses, its cell check made for K1 taps; a NULL tail; a mix_time_s, fade_s or gain that is negative or not
 * finite; reserved != 0; s0 not finite or above 1024.  GAS_ERR_UNSUPPORTED_CHAIN and GAS_ERR_DEVICE: as for the *_bands
 * calls.
 * Out of scope: jitter of individual images, a diffuse-field-equalised colouring of the tail, interaural coherence of
 * the diffuse part, a fitted hand-over level, the host layer, godot_module/ and gas_multi. */
typedef struct gas_room_tail { /* NEW; 32 bytes */
	uint32_t seed; /* any value; selects the noise */
	float mix_time_s; /* >= 0, finite: the cross-fade begins this long after the direct sound */
	float fade_s; /* >= 0, finite: its length; 0 = a hard switch */
	float gain; /* >= 0, finite: linear trim of the diffuse part; 1 = the rule's level */
	uint32_t reserved[4]; /* 0 */
} gas_room_tail;
int gas_conv_ir_from_room_diffuse(gas_ctx *ctx, const gas_room_ir *desc, const gas_room_bands *bands, const gas_room_tail *tail, uint32_t channels /* 1 or 2 */, uint32_t taps, float *out_taps /* host [channels][taps], may be NULL */, uint32_t *out_ir /* may be NULL */);
int gas_conv_ir_from_room_hrtf_diffuse(gas_ctx *ctx, const gas_room_ir *desc, const gas_room_bands *bands, const gas_room_tail *tail, const float *hrir /* host [n_az * n_el][2 ears][hrir_taps] f32 */, uint32_t n_az, uint32_t n_el, uint32_t hrir_taps /* 1 .. GAS_HRTF_TAPS */, uint32_t taps, float *out_taps /* host [2][taps], may be NULL */, uint32_t *out_ir /* may be NULL */);


/* ---- device-resident source sampling ------------------------------------------------
 * The step in front of the path: AudioStreamPlayback::mix into the 64-frame lookahead window with the
 * end-of-stream fade-out (audio_spatializer.cpp:367-408), over PCM that already lives in HBM, so a callback
 * moves no source frames over PCIe.  Streams are 16-bit PCM as in the reference's example asset
 * (speech_orig.wav: mono, 16-bit, 48 kHz); samples convert as s / 32768, mono feeds both ears [ENGINE].
 * Streams are taken to be at the context's mix rate; pitch-scaled playback: gas_stream_set_resampled. */
typedef enum gas_pcm_format {
	GAS_PCM_S16 = 0, /* interleaved little-endian int16 */
	GAS_PCM_F32 = 1, /* interleaved float32 (already decoded) */
	GAS_PCM_IMA_ADPCM = 2, /* 4-bit IMA/DVI ADPCM codes, see below */
	GAS_PCM_QOA = 3, /* a whole QOA ("Quite OK Audio") file, see below */
} gas_pcm_format;
/* GAS_PCM_IMA_ADPCM.  The data are [ENGINE] AudioStreamWAV's FORMAT_IMA_ADPCM data as stored (recollection of the engine
 * source, parity unpinned): one 4-bit code per frame and channel, channel c's frame i in byte (i >> 1) * channels + c,
 * low nibble for even i, high nibble for odd i; no block headers; the call reads ((frames + 1) / 2) * channels bytes.
 * The decoder is the public IMA/DVI standard.  Per channel (predictor, step_index) = (0, 0) before frame 0; per code n:
 *   step = STEP[step_index];  step_index = clamp(step_index + INDEX[n & 7], 0, 88)
 *   diff = step >> 3, + step >> 2 if n & 1, + step >> 1 if n & 2, + step if n & 4; negated if n & 8
 *   predictor = clamp(predictor + diff, -32768, 32767); the sample is predictor
 * with the standard 89-entry STEP table (7 ... 32767) and INDEX = {-1, -1, -1, -1, 2, 4, 6, 8}.
 * In every entry a stream of this format behaves exactly as the GAS_PCM_S16 stream of its decoded samples would
 * (resampled, looped in both modes -- decoding is random-access here --, bound at any start_frame).
 * Device memory: the codes plus the decoder state in front of every 32 frames (4 bytes per channel), 20 bytes per 32
 * samples = 5 bits per sample, counted in whole 32-frame chunks. */
/* GAS_PCM_QOA.  The data are [ENGINE] AudioStreamWAV's FORMAT_QOA data as stored, taken to be the whole QOA file
 * (recollection of the engine source, parity unpinned).  The format is the public QOA specification; all fields are
 * big-endian:
 *   file header   'qoaf', u32 samples per channel
 *   frames        ceil(samples / 5120) of them, each
 *     header      u8 channels, u24 sample rate, u16 fsamples (samples per channel in this frame), u16 fsize (bytes of the
 *                 frame, header included)
 *     state       per channel history[4] int16, then weights[4] int16 (16 bytes per channel)
 *     slices      ceil(fsamples / 20) per channel, interleaved by channel (slice s of channel 0, slice s of channel 1,
 *                 slice s + 1 of channel 0, ...);  fsize = 8 + 16 * channels + 8 * slices * channels
 *   slice         a u64: bits 63..60 the scale factor sf, then 20 residual codes of 3 bits, the first in bits 59..57; a
 *                 partial last slice is padded with zeros
 * The call reads the bytes that `frames` and `channels` imply (8 + the sum of the fsize values) and validates before it
 * uploads anything; GAS_ERR_INVALID_ARGUMENT, and no stream, if the magic is not 'qoaf' (checked before anything else is
 * read), the header's sample count is not `frames`, a frame header's channel count is not `channels` (1 or 2 only), or
 * a frame header's fsamples or fsize is not what the layout implies.  The sample-rate fields are ignored: streams are
 * taken to be at the context's mix rate.
 * The decoder is a 4-tap sign-LMS predictor.  Every frame header RELOADS (h, w) = (history, weights) of each channel --
 * nothing carries across a frame edge -- and per sample, in 32-bit two's-complement arithmetic that wraps:
 *   p = (w0 * h0 + w1 * h1 + w2 * h2 + w3 * h3) >> 13          (arithmetic shift)
 *   d = DEQ[sf][code];  s = clamp(p + d, -32768, 32767);  delta = d >> 4
 *   w[i] += (h[i] < 0 ? -delta : delta);  h = (h1, h2, h3, s);  the sample is s
 * with DEQ[sf][k] = round-half-away-from-zero of round((sf + 1)^2.75) * {0.75, -0.75, 2.5, -2.5, 4.5, -4.5, 7, -7}[k]
 * (scale factors 1, 7, 21, 45, 84, 138, 211, 304, 421, 562, 731, 928, 1157, 1419, 1715, 2048).
 * In every entry a stream of this format behaves exactly as the GAS_PCM_S16 stream of its decoded samples would
 * (resampled, looped in both modes, bound at any start_frame, positions, the host layer).
 * Device memory: one 64-byte record per 80 frames (4 slices) and channel -- the slices as stored and the decoder state
 * in front of them, filled by one decode on the host in this call -- 6.4 bits per sample, counted in whole 80-frame
 * chunks. */

int gas_stream_create(gas_ctx *ctx, const void *pcm, int format, uint32_t channels /* 1 or 2 */, uint64_t frames, uint32_t *out_stream);
/* Which engine playback class stands behind the stream's playbacks (choose before binding them):
 *   off (default): frames are handed out as they are; pitch_scale must be 1 (or 0 = unset), anything else is
 *                  GAS_ERR_UNSUPPORTED_CHAIN;
 *   on:            [ENGINE] AudioStreamPlaybackResampled::mix (audio_spatializer.cpp:375-378 passes pitch_scale per
 *                  playback and callback; audio_spatializer_3d.cpp:405-434 sets it from doppler): a 16.16 fixed-point
 *                  position advanced by pitch_scale per output frame and 4-point cubic interpolation over the frames
 *                  q-3 .. q, at ANY pitch including 1 (where it is a 2-frame delay).  Recollection of the engine source,
 *                  parity unpinned; the stream is taken to be at the context's mix rate.  pitch_scale is the value last
 *                  published from the host (gas_params_publish*); 0 <= pitch_scale < 32768. */
int gas_stream_set_resampled(gas_ctx *ctx, uint32_t stream, int on);
/* NEW (no counterpart in the reference; named after [ENGINE] AudioStreamWAV's loop modes, not a restatement of its
 * mixer): the stream's playbacks repeat [loop_begin, loop_end).  A looped playback behaves exactly as a plain playback
 * over the unrolled stream U[k] = S[m(k)], k = 0, 1, 2, ...; with b = loop_begin, e = loop_end, L = e - b:
 *   k <  b: m(k) = k
 *   k >= b: t = (k - b) mod P;  FORWARD: P = L, m = b + t;  PINGPONG: P = 2L, m = b + (t < L ? t : 2L - 1 - t)
 * (both end frames of a ping-pong loop play twice; frames from e on never play).  Cursor, 64-frame lookahead, the
 * resampler's taps and start_frame all count on the unrolled timeline; no fade at a seam; the playback never ends on
 * its own (has_frames stays 1) and stops through gas_source_set_draining / gas_source_free like any other.
 * loop_end == 0 means the stream's length.  Chosen before playbacks are bound, like gas_stream_set_resampled: a bound
 * stream answers GAS_ERR_INVALID_ARGUMENT, an unknown one GAS_ERR_BAD_SLOT.  An unknown mode, loop_begin >= loop_end,
 * loop_end > frames and L >= 2^31 answer GAS_ERR_INVALID_ARGUMENT and change nothing.  GAS_LOOP_DISABLED ignores
 * loop_begin / loop_end. */
typedef enum gas_loop_mode {
	GAS_LOOP_DISABLED = 0,
	GAS_LOOP_FORWARD = 1,
	GAS_LOOP_PINGPONG = 2,
} gas_loop_mode;
int gas_stream_set_loop(gas_ctx *ctx, uint32_t stream, int mode, uint64_t loop_begin, uint64_t loop_end);
/* The stream's loop as set (DISABLED: begin = end = 0; any of the outputs may be NULL). */
int gas_stream_get_loop(gas_ctx *ctx, uint32_t stream, int *out_mode, uint64_t *out_begin, uint64_t *out_end);
int gas_stream_destroy(gas_ctx *ctx, uint32_t stream);
/* Length, channel count and sample format of a stream (any of the outputs may be NULL). */
int gas_stream_get_info(gas_ctx *ctx, uint32_t stream, uint64_t *out_frames, uint32_t *out_channels, int *out_format);
/* start_playback_stream (audio_spatializer.cpp:55-63): the slot's playback starts at start_frame of the stream
 * with a zeroed lookahead and has_frames set.  For a looped stream start_frame is a position on the unrolled
 * timeline and is not clamped to the stream's length. */
int gas_source_bind_stream(gas_ctx *ctx, uint32_t slot, uint32_t stream, uint64_t start_frame);
/* Like gas_process_block, but the source windows are produced on the device from the bound streams (cursor
 * advance, lookahead delay, fade-out, zero feed after the end).  has_frames ([n] bytes, host, may be NULL)
 * receives each playback's has_frames flag after this callback (audio_spatializer.cpp:398); slots whose
 * stream ended are marked draining automatically.  out / peaks are host or device pointers per `mem`. */
int gas_process_block_streams(gas_ctx *ctx, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out, float *peaks, uint8_t *has_frames, int mem);
/* gas_process_block_buses over the windows gas_process_block_streams would have produced for the same list: every
 * playback mixes onto its dry bus and its sends (gas_bus_routes_publish) without a source frame crossing to the device.
 *   From the streams entry: cursor advance and lookahead delay, the fade-out at a stream's end and zeros after it,
 *     automatic draining, has_frames, the resampled-pitch rules (GAS_ERR_UNSUPPORTED_CHAIN for pitch != 1 on a
 *     non-resampled stream), GAS_ERR_INVALID_ARGUMENT for one slot twice.
 *   From the bus entry: 1 <= n_buses <= GAS_MAX_BUSES; the routes snapshot; either every source GAS_KIND_3D_MIX, or every
 *     source a non-empty effect chain on a one-pair context (anything else: GAS_ERR_UNSUPPORTED_CHAIN); peaks are those
 *     of y before any bus factor; out ([n_buses][C][frames]) is fully overwritten, with zeros when n == 0.
 * `mem` governs out and peaks.  A failed callback moves no cursor: everything either entry can refuse for the list
 * (n_buses, the kinds, an empty chain, a chain on C > 1, GAS_ERR_NO_HRTF, GAS_ERR_NO_PARAMS, a duplicate) is checked
 * before the sampler runs, and a host `out` comes back zeroed (n_buses out of range: its first
 * min(n_buses, GAS_MAX_BUSES) buses).
 * Routes: plain [HRTF] lists of uncompressed, non-resampled streams on a one-pair context are sampled inside the HRTF
 * kernel (k_hrtf_uni<SRC_PCM, BUS2>, one launch per pair of buses, the cursors committed by the last); every other
 * list the bus entry accepts (3D mix on 1..4 pairs, staged chains, resampled / ADPCM / QOA / blend-fade playbacks) has
 * its rows sampled first and runs the device path of gas_process_block_buses over them. */
int gas_process_block_streams_buses(gas_ctx *ctx, const uint32_t *slots, uint32_t n, uint32_t frames, gas_audio_frame *out /* [n_buses][C][frames] */, uint32_t n_buses, float *peaks, uint8_t *has_frames, int mem);
/* Where the playbacks of the LAST stream callback's list (gas_process_block_streams or gas_process_block_streams_buses,
 * whichever ran last) stand in their streams after it, in its row order:
 * out_frames[i] = index of the next stream frame playback i will take ([ENGINE] get_playback_position x mix rate, plus
 * the playback's start frame; for a looped stream m(k) of the frames consumed).  From the host-side mirror of the cursor arithmetic: nothing is read back from the
 * device.  n must be that callback's n.  Audio thread. */
int gas_stream_positions(gas_ctx *ctx, uint32_t n, uint64_t *out_frames);
/* NEW.  The 64-frame-delayed window (what gas_process_block's src row holds) of playbacks that are NOT bound to a
 * stream, for the next stream callback: a playback the host decodes (Ogg Vorbis, MP3, a generator, a microphone) next
 * to device-resident ones, in one list and one fixed-order mix.
 *   rows      [n][frames] frames of `format` (GAS_PCM_S16 or GAS_PCM_F32 only) and `channels` (1 or 2), row i for
 *             slots[i].  Converted as streams are: s / 32768, mono feeds both ears.
 *   mem       GAS_MEM_HOST: `rows` has been consumed when the call returns -- copied into pinned staging (which grows
 *             to the largest call made so far, so not in the steady state) and uploaded from there; the call waits only
 *             while the previous call's upload is still queued.  GAS_MEM_DEVICE: the call enqueues a device copy in the
 *             context's stream order, as gas_sidechain_set does: `rows` need only be valid at that point of the stream.
 *             Callbacks recorded or deferred under GAS_FLAG_BATCHED_LAUNCH run first.
 * In the next gas_process_block_streams / gas_process_block_streams_buses that passes its validation, a list entry whose
 * slot has a pending row takes that row as its window, reports has_frames = 1, is not auto-marked draining (a mark an
 * earlier, unfed callback left stays until gas_source_set_draining clears it), moves no cursor and reports 0 in
 * gas_stream_positions.  The callback's mix, peaks and bus outputs are those of gas_process_block[_buses] over the rows
 * R, R[i] the sampler's window where entry i is a stream playback and the converted fed row where it is fed.
 * A pending row: the callback that uses it consumes it (one feed serves one callback); a later feed of the same slot
 * before that callback replaces it, and several calls accumulate; a callback that fails validation leaves it where it
 * is, as it leaves the cursors; that callback drops the pending row of a slot its list does not name;
 * gas_source_free, gas_source_reset and gas_source_bind_stream of the slot drop it.  An unbound slot without a pending
 * row behaves as ever: a silent row, has_frames = 0, marked draining.
 * Routes: a plain [HRTF] list keeps its one-launch forms with fed entries (k_hrtf_uni<SRC_PCM> and
 * k_hrtf_uni<SRC_PCM, BUS2> read a fed row as a stream window); on a cross-fade, direction-run, direction-order or
 * interpolation context -- the k_hrtf_ols stream-sampling forms -- a callback with a fed entry samples its rows first.
 * Errors, each leaving nothing taken: GAS_ERR_INVALID_ARGUMENT for a bad format, channels or mem, a slot bound to a
 * stream, a slot named twice in one call; GAS_ERR_BAD_SLOT for a slot that is not in use; GAS_ERR_FRAME_COUNT for
 * frames != cfg.frames; GAS_ERR_DEVICE for a HIP failure (GAS_ERR_OUT_OF_MEMORY when the feed table -- header + 2 x max_sources float32 stereo rows of device
 * memory, allocated by the first call -- or the pinned staging cannot be allocated).  pitch_scale of a playback that is
 * bound to no stream is not looked at by the stream callbacks: whoever decodes it has applied it, as for the rows of
 * gas_process_block.
 * Audio thread. */
int gas_source_feed_rows(gas_ctx *ctx, const uint32_t *slots, const void *rows /* [n][frames] */, int format, uint32_t channels, uint32_t n, uint32_t frames, int mem);
/* Diagnostic: 1 if the last stream callback that reached its launches sampled its windows inside the HRTF kernel (the
 * fused route), 0 if it sampled rows first; GAS_ERR_INVALID_ARGUMENT for ctx == NULL. */
int gas_stream_last_fused(gas_ctx *ctx);

/* ---- measurement ------------------------------------------------------- */
/* on = 0 off, 1 = bracket the dominant launch of every callback with HIP events, N > 1 = of every Nth callback. */
int gas_profile_enable(gas_ctx *ctx, int on);
int gas_profile_read(gas_ctx *ctx, gas_profile *out, int reset);
/* Same-run copy-bandwidth ceiling: a pure streaming launch (16-byte loads of read_bytes from an arena
 * larger than the Infinity Cache, 16-byte stores of write_bytes) timed with the same HIP-event bracket and marker
 * calibration as the dominant kernel; *out_us = average span of one launch on the GPU timeline over `iters` launches.
 * workgroups x 256 threads, `unroll` (1, 2, 4 or 8) independent loads in flight per thread. */
int gas_bandwidth_probe(gas_ctx *ctx, uint64_t read_bytes, uint64_t write_bytes, uint32_t workgroups, uint32_t unroll, uint32_t iters, double *out_us);
/* Tuning (process-wide, not per context): plain-[HRTF] callbacks of at least `min_sources` float-row sources on one
 * bus run k_hrtf_uni's twelve-wave form (three waves per SIMD, HRIR rows staged through LDS); 0 = never.  The two
 * forms split the sources over waves differently, so their mixes agree to rounding (1e-5 relative RMS), not to
 * the bit.  The build's default: DESIGN.md 3.1; environment variable GAS_UNI12_MIN overrides it at load time.
 * Returns the previous value. */
uint32_t gas_tune_uni12_min(uint32_t min_sources);
/* Tuning (process-wide): plain-[HRTF] callbacks of at least `min_sources` sources read and write their history rows
 * with non-temporal accesses (rows too many to survive in the Infinity Cache from one callback to the next; default
 * 196608, environment variable GAS_NT_HIST_MIN).  A cache hint only: results do not change.  Returns the previous value. */
uint32_t gas_tune_nt_hist_min(uint32_t min_sources);
/* Diagnostic: the processing order the last gas_process_block used for its plain [HRTF] sources (GAS_FLAG_XCD_ORDER
 * only): out[i] = list entry processed i-th; waits for the stream.  GAS_ERR_INVALID_ARGUMENT when that
 * callback ran in list order. */
int gas_ctx_read_hrtf_order(gas_ctx *ctx, uint32_t *out, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif /* GAS_AMD_H */
