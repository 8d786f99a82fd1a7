/*
 * hartallo_amd.h -- C ABI of the MI355X (gfx950) H.264 encode path.
 *
 * Drop-in boundary.  hartallo reaches an encoder through one plugin slot:
 *
 *   HL_ERROR_T (*encode)(struct hl_codec_s*, const struct hl_frame_s*,
 *                        struct hl_codec_result_s*);
 *     include/hartallo/hl_codec.h:173-184 (hl_codec_plugin_def_t.encode),
 *     called by hl_codec_encode, source/hl_codec.c:152-159.
 *
 * The H.264 plugin behind it (hl_codec_264_encode, source/h264/
 * hl_codec_264.c:637-1006) turns one planar YUV420 frame into headers +
 * one slice NAL.  The functions below are that operation with plain C types:
 * a maintainer registers a plugin def whose encode() forwards here (see
 * INTEGRATION.md), and hartallo's public API is unchanged.
 *
 * Semantics follow the reference:
 *   - parameters are the hl_codec_t fields the encoder reads
 *     (hl_codec.h:33-80): qp, gop_size, me_range, deblock_flag,
 *     me_early_term_flag; max_ref_frame through hl_amd_set_max_ref_frame;
 *     threads_count is 1 (the reference cuts a picture into threads_count
 *     slices, hl_codec_264.c:571; one slice per picture here);
 *   - width and height must be multiples of 16 (1088, not 1080 -- the
 *     reference rejects cropping, hl_codec_264.c:430-438);
 *   - result.type carries HL_CODEC_RESULT_TYPE_DATA / _HDR bits
 *     (hl_types.h:158-163); result.hdr holds "00 00 01"-prefixed SPS+PPS
 *     on the first frame (hl_codec_264.c:675-686), result.data the slice
 *     NAL without its start code (hl_codec_264.c:1000-1006);
 *   - the output buffers are owned by the encoder and valid until the next
 *     call (hl_codec_264.c:1000-1006);
 *   - errors are HL_ERROR_T values (hl_types.h:101-122).
 * Output is bit-identical to the reference encoder on the same input.
 */
#ifndef HARTALLO_AMD_H
#define HARTALLO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* HL_ERROR_T values, hl_types.h:101-122 */
enum {
    HL_AMD_SUCCESS = 0,
    HL_AMD_ERROR_INVALID_PARAMETER = 1,
    HL_AMD_ERROR_INVALID_STATE = 3,
    HL_AMD_ERROR_INVALID_FORMAT = 4,
    HL_AMD_ERROR_NOT_FOUND = 6,
    HL_AMD_ERROR_NOT_IMPLEMENTED = 7,
    HL_AMD_ERROR_OUTOFMEMMORY = 8,
    HL_AMD_ERROR_OUTOFCAPACITY = 10,
    HL_AMD_ERROR_SYSTEM = 13,
    HL_AMD_ERROR_TOOSHORT = 15
};

/* HL_CODEC_RESULT_TYPE_T bits, hl_types.h:158-163 */
enum { HL_AMD_RESULT_TYPE_DATA = 1, HL_AMD_RESULT_TYPE_HDR = 2 };

typedef struct hl_amd_params_s {
    int32_t width;          /* hl_codec_t.width  (multiple of 16) */
    int32_t height;         /* hl_codec_t.height (multiple of 16) */
    int32_t qp;             /* hl_codec_t.qp, 0..51 */
    int32_t me_range;       /* hl_codec_t.me_range, clipped to [1,64] (rdo.c:847) */
    int32_t deblock;        /* hl_codec_t.deblock_flag */
    int32_t gop_size;       /* hl_codec_t.gop_size */
    int32_t me_early_term;  /* hl_codec_t.me_early_term_flag (homogeneity mode masks,
                               rdo.c:888-931); 1 needs width and height >= 32 */
    int32_t device;         /* HIP device ordinal */
} hl_amd_params_t;

typedef struct hl_amd_result_s {
    int32_t type;            /* HL_AMD_RESULT_TYPE_* bits */
    const uint8_t* hdr;      /* SPS + PPS with start codes, when type & HDR */
    size_t hdr_size;
    const uint8_t* data;     /* slice NAL without start code, when type & DATA */
    size_t data_size;
} hl_amd_result_t;

typedef struct hl_amd_encoder_s hl_amd_encoder_t;

/* hl_codec_create + option setting for HL_CODEC_TYPE_H264 (hl_codec.c:24-150).
 * A/B knob read here: HL_AMD_MEMO -- the memo of the per-block candidate
 * evaluation: unset = the built capacity, 0 = off, N = N slots
 * (a power of two up to the capacity; anything else: INVALID_PARAMETER).
 * Results do not depend on it. */
int32_t hl_amd_encoder_create(const hl_amd_params_t* params, hl_amd_encoder_t** encoder);
void hl_amd_encoder_destroy(hl_amd_encoder_t* encoder);

/* plugin encode() for a planar YUV420 frame in host memory
 * (hl_frame_video_t data_ptr[0..2], hl_frame.h:278-291) */
int32_t hl_amd_encode(hl_amd_encoder_t* encoder, const uint8_t* y, const uint8_t* u, const uint8_t* v,
                      hl_amd_result_t* result);

/* Look-ahead for per-frame callers (no reference interface: hl_codec_encode,
 * hl_codec.c:152-159, codes one frame per call and has no flush).  With
 * frames = k > 1, set before the first frame: hl_amd_encode queues each host
 * frame in device memory and codes every k queued frames as one
 * hl_amd_encode_batch (a frame-pipelined run); each call hands out the next
 * coded result in order -- type 0 (nothing) while the first k - 1 frames
 * queue, so a frame's bytes come k - 1 calls later -- and hl_amd_flush codes
 * what is still queued and hands out the remaining results, one per call,
 * type 0 once none is left.  The bytes are those of k separate calls.  An
 * error is reported by the call that codes the batch.  k = 1: off (the
 * default).  AVC only (adding a layer turns it off).  While frames are
 * queued, hl_amd_encode_device and hl_amd_encode_batch are refused
 * (HL_AMD_ERROR_INVALID_STATE): flush first. */
int32_t hl_amd_set_lookahead(hl_amd_encoder_t* encoder, int32_t frames);
int32_t hl_amd_flush(hl_amd_encoder_t* encoder, hl_amd_result_t* result);

/* same, with the planes already resident in device memory (HBM) */
int32_t hl_amd_encode_device(hl_amd_encoder_t* encoder, const uint8_t* y, const uint8_t* u, const uint8_t* v,
                             hl_amd_result_t* result);

/* n consecutive frames of the stream (planes resident in device memory),
 * encoded as if by n calls of hl_amd_encode_device, with results[i] the
 * i-th call's result (bitstreams identical).  Runs of P pictures are encoded
 * in one frame-pipelined launch: picture f+1 starts as soon as picture f has
 * finished the region its motion search can reach.  The data of every
 * result stays valid until the next call on this encoder.  No reference
 * interface: a throughput entry point for callers that hold several frames
 * (hl_codec_encode takes one frame per call, hl_codec.c:152-159). */
int32_t hl_amd_encode_batch(hl_amd_encoder_t* encoder, int32_t n, const uint8_t* const* y, const uint8_t* const* u,
                            const uint8_t* const* v, hl_amd_result_t* results);

/* n frames of each of `count` independent streams (1..16 encoders, one per
 * stream: the same picture size and device, no rate control, no spatial
 * layers) in shared pipelined runs: one persistent launch holds every
 * stream's pictures, so the streams' macroblock tasks share the device's
 * workgroups and one stream's wavefront ramp and tail overlap the others'
 * work (several streams per GPU without processes time-slicing the device).
 * y[s * n + i] = frame i of stream s (device memory, as hl_amd_encode_batch);
 * results[s * n + i] its result, valid until the next call on that encoder;
 * each stream's results are those of hl_amd_encode_batch on its encoder
 * alone (the reference serves N streams as N hl_codec_t instances,
 * hl_codec.c:24-150).  The diagnostics of every encoder (stats, timing)
 * describe the shared launches, and encoder 0's pipeline settings
 * (hl_amd_set_pipeline, hl_amd_set_intra_helpers, hl_amd_set_timing) govern
 * them.  The streams advance together: an error before any stream commits
 * leaves every encoder as it was; a stream whose picture-by-picture fallback
 * fails after others committed leaves every encoder of the call unusable
 * (HL_AMD_ERROR_INVALID_STATE from then on).  No reference interface. */
int32_t hl_amd_encode_streams(hl_amd_encoder_t* const* encoders, int32_t count, int32_t n, const uint8_t* const* y,
                              const uint8_t* const* u, const uint8_t* const* v, hl_amd_result_t* results);

/* ---- per-frame encoding type and live settings ----
 * What the reference reads on every hl_codec_encode call beside the planes:
 * hl_frame_t.encoding (hl_frame.h:38-39, HL_VIDEO_ENCODING_TYPE_T,
 * hl_types.h:262-274) and the hl_codec_t fields it never snapshots.  The
 * hl_amd_*_ex calls take them per frame; a NULL ctl is the call without _ex
 * (AUTO, settings as they are).
 *   - picture type (hl_codec_264.c:705-718): a GOP counter that has run out
 *     gives an IDR whatever is asked and reloads from gop_size; else AUTO and
 *     INTER give a P picture and INTRA gives an IDR and reloads the counter
 *     from gop_size.  frame_num goes on counting (encode.c:251), idr_pic_id
 *     counts every IDR (encode.c:527-530), SPS / PPS are not sent again;
 *   - me_range (rdo.c:847), deblock (slice.c:1897, the slice header's
 *     disable_deblocking_filter_idc, slice.c:1739) and me_early_term
 *     (rdo.c:889) apply from the call that carries them and stay until the
 *     next _ex call changes them; gop_size likewise, and is read only where
 *     the counter reloads (hl_codec_264.c:709, 717);
 *   - qp is not here: the reference captures it at the first frame
 *     (hl_codec_264.c:465) and ignores later changes;
 *   - under rate control a forced IDR starts a GOP of the model as a
 *     scheduled one does (hl_codec_264.c:723-737);
 *   - RAW (I_PCM, whose reference output is truncated: hl_codec_264_mb.c:
 *     247-310 overruns its bit buffer), LOSSLESS (no case in encode.c:230 and
 *     slice.c:1819) and unknown values: HL_AMD_ERROR_NOT_IMPLEMENTED.
 *     me_early_term on a picture under 32x32 (rdo.c:895-896):
 *     HL_AMD_ERROR_INVALID_PARAMETER.  Every ctl of a call is checked before
 *     anything is coded or queued, and a refused call leaves the encoder as
 *     it was: the next call continues the stream;
 *   - an encoder with layers (hl_amd_add_layer) accepts a ctl only with AUTO
 *     or INTER and the settings it was created with, else
 *     HL_AMD_ERROR_NOT_IMPLEMENTED;
 *   - look-ahead: every queued frame keeps its ctl; the bytes are those of k
 *     separate hl_amd_encode_ex calls.
 * In hl_amd_encode_batch_ex / hl_amd_encode_streams_ex a forced IDR or a
 * changed setting stays inside the frame-pipelined run: every picture of a
 * run carries its own type and settings. */
enum {
    HL_AMD_ENCODING_AUTO = 0,
    HL_AMD_ENCODING_INTRA,
    HL_AMD_ENCODING_INTER,
    HL_AMD_ENCODING_LOSSLESS,
    HL_AMD_ENCODING_RAW
}; /* = HL_VIDEO_ENCODING_TYPE_T */

typedef struct hl_amd_frame_ctl_s {
    int32_t encoding;       /* HL_AMD_ENCODING_* (hl_frame_t.encoding) */
    int32_t me_range;       /* the hl_codec_t values at the time of this frame's call */
    int32_t deblock;
    int32_t me_early_term;
    int32_t gop_size;
} hl_amd_frame_ctl_t;

int32_t hl_amd_encode_ex(hl_amd_encoder_t* encoder, const uint8_t* y, const uint8_t* u, const uint8_t* v,
                         const hl_amd_frame_ctl_t* ctl, hl_amd_result_t* result);
int32_t hl_amd_encode_device_ex(hl_amd_encoder_t* encoder, const uint8_t* y, const uint8_t* u, const uint8_t* v,
                                const hl_amd_frame_ctl_t* ctl, hl_amd_result_t* result);
/* ctl: n entries, frame by frame */
int32_t hl_amd_encode_batch_ex(hl_amd_encoder_t* encoder, int32_t n, const uint8_t* const* y, const uint8_t* const* u,
                               const uint8_t* const* v, const hl_amd_frame_ctl_t* ctl, hl_amd_result_t* results);
/* ctl: count * n entries, ctl[s * n + i] = frame i of stream s */
int32_t hl_amd_encode_streams_ex(hl_amd_encoder_t* const* encoders, int32_t count, int32_t n, const uint8_t* const* y,
                                 const uint8_t* const* u, const uint8_t* const* v, const hl_amd_frame_ctl_t* ctl,
                                 hl_amd_result_t* results);

/* rate control (hl_codec_t.rc_bitrate > 0; hl_codec_264.c:719-742, 1018-1031,
 * model hl_codec_264_rc.c): bitrate in bits/s, frame rate fps_den / fps_num
 * (hl_codec_t.fps, integer quotient), rc_basicunit (<= 0: the picture),
 * rc_qp_min / rc_qp_max (-1: 0 / 51).  Call before the first frame;
 * bitrate <= 0 turns it off.  Each picture's QP then follows the previous
 * pictures' bits, so hl_amd_encode_batch codes the pictures one by one. */
int32_t hl_amd_set_rate_control(hl_amd_encoder_t* encoder, int64_t bitrate, int32_t fps_num, int32_t fps_den,
                                int32_t basicunit, int32_t qp_min, int32_t qp_max);

/* hl_codec_t.max_ref_frame (hl_codec.c:36, default 1): the SPS's
 * max_num_ref_frames = min(MaxDpbMbs / PicSizeInMbs, max_ref_frame)
 * (hl_codec_264_sps.c:620-636) and the PPS's
 * num_ref_idx_l0_default_active_minus1 (hl_codec_264_pps.c:291), for every
 * (subset) SPS / PPS of the stream.  The reference's P slices override the
 * active references to one (slice.c:289, encode.c:269), so only the headers
 * change.  Any value >= 0 (the reference takes any and writes the clamped
 * one: 720p with 32 gives 5); HL_AMD_ERROR_INVALID_PARAMETER only when the
 * clamped value is above 16.  Call before the first frame (the reference
 * reads it when it builds the first SPS), else HL_AMD_ERROR_INVALID_STATE. */
int32_t hl_amd_set_max_ref_frame(hl_amd_encoder_t* encoder, int32_t max_ref_frame);

/* ---- pictures of any even size: the display size ----
 * No reference interface: the reference refuses pictures that are no
 * multiples of 16 (hl_codec_264.c:430-433) and always writes
 * frame_cropping_flag = 0 (hl_codec_264_sps.c:625).  The encoder is created
 * at the coded size W x H (multiples of 16, as ever); the display size dw x dh
 * -- both even, W - 16 < dw <= W, H - 16 < dh <= H, else
 * HL_AMD_ERROR_INVALID_PARAMETER -- is what a decoder shows: the SPS then
 * carries frame_cropping_flag = 1 with the offsets left 0, right (W - dw) / 2,
 * top 0, bottom (H - dh) / 2 (units of two luma samples), and every other
 * field, level_idc and max_num_ref_frames included, stays the reference's for
 * W x H.  The PPS and every slice NAL are the reference's for the coded
 * picture, byte for byte.  (W, H) means none: today's headers.  Off by
 * default; it changes no byte of a stream coded without it.
 * Which call takes which size:
 *   - hl_amd_encode, _device, _batch, _streams and their _ex forms keep taking
 *     planes of the coded size that the caller padded;
 *   - hl_amd_encode_frame and hl_amd_encode_frames take frames of the display
 *     size (rows and row bytes follow dw and dh) and the encoder pads them to
 *     W x H on the GPU by edge replication of the converted planes, defined
 *     through clamped coordinates: luma sample (x, y) is the converted luma of
 *     source sample (min(x, dw - 1), min(y, dh - 1)), chroma sample (bx, by)
 *     the converted chroma of source 2x2 block (min(bx, dw/2 - 1),
 *     min(by, dh/2 - 1)) -- for RGB that block's SR, SG, SB through the
 *     arithmetic below.  Scene-cut detection reads the padded planes;
 *   - hl_amd_get_input, hl_amd_get_recon and the debug calls return planes of
 *     the coded size (no cropping is applied to them);
 *   - quality (hl_amd_set_quality) measures the display rectangle only: dw x dh
 *     of luma, dw/2 x dh/2 of chroma (see there).
 * Like hl_amd_set_max_ref_frame it is part of the SPS: accepted only before
 * the first picture and with nothing queued in the look-ahead, else
 * HL_AMD_ERROR_INVALID_STATE; the two setters work in either order.  Encoders
 * with spatial layers: HL_AMD_ERROR_NOT_IMPLEMENTED, and hl_amd_add_layer
 * after a display size was set returns the same.  Not served: left and top
 * offsets, odd sizes, a VUI. */
int32_t hl_amd_set_display_size(hl_amd_encoder_t* encoder, int32_t width, int32_t height);
/* the display size (the coded size when none was set) */
int32_t hl_amd_get_display_size(hl_amd_encoder_t* encoder, int32_t* width, int32_t* height);

/* The SPS and PPS ("00 00 01"-prefixed) that an encoder created with these
 * parameters (width, height and qp are read) emits after
 * hl_amd_set_max_ref_frame(max_ref_frame) and hl_amd_set_display_size(
 * display_width, display_height) -- (width, height) for no cropping.  A pure
 * function (no device).  Returns the bytes written, or 0 when a setting is
 * refused or the bytes do not fit in cap. */
size_t hl_amd_stream_headers(const hl_amd_params_t* params, int32_t max_ref_frame, int32_t display_width, int32_t display_height,
                             uint8_t* out, size_t cap);

/* SliceQPY of the last encoded picture (the rate-controlled QP), or -1 */
int32_t hl_amd_last_qp(hl_amd_encoder_t* encoder);

/* pipelined-run scheduling: persistent workgroups (0 = one per resident
 * workgroup slot of the device, <= 4096), the reference reach R in MBs
 * (0..16) that a macroblock task of picture f+1 waits for in picture f
 * before it becomes ready, and the pictures (1..64, from the oldest
 * unfinished one) a workgroup looks at for ready tasks; defaults 0, 2, 64.
 * Results do not depend on these. */
int32_t hl_amd_set_pipeline(hl_amd_encoder_t* encoder, int32_t workgroups, int32_t reach, int32_t window);

/* resident workgroups per CU of the pipelined kernel (HIP occupancy query;
 * geometry tuning), or -1 */
int32_t hl_amd_pipeline_occupancy(void);

/* Which build of the pipelined kernel a run launches: 0 = chosen per run
 * (the default), 1 = 512-lane workgroups (one macroblock per CU), 2 = 256-lane
 * workgroups (two macroblocks per CU) for every run of more than one picture.
 * A lone picture keeps the build with the 8x8-family helper tasks whatever
 * the mode.  hl_amd_encode_streams follows its first encoder's mode.
 * Results do not depend on it. */
int32_t hl_amd_set_pipeline_build(hl_amd_encoder_t* encoder, int32_t mode);

/* the build the last pipelined run launched: 0 = with the 8x8-family helper
 * tasks (512 lanes), 1 = 512-lane, 2 = 256-lane; -1 before any run */
int32_t hl_amd_last_pipeline_build(hl_amd_encoder_t* encoder);

/* The launcher's choice (a pure function; no device): the build -- as
 * hl_amd_last_pipeline_build reports it -- of a run that holds `pictures`
 * pictures over all its streams, under `mode`, where `fam3` says that the run
 * qualifies for the 8x8-family helper tasks.  -1 for an invalid argument. */
int32_t hl_amd_pipeline_build_choice(int32_t mode, int32_t pictures, int32_t fam3);

/* pictures of a run from which mode 0 picks the 256-lane build; 0 = never */
int32_t hl_amd_pipeline_build_threshold(void);

/* reconstructed (deblocked) picture of the last encoded frame, i.e. the
 * reference picture the next frame predicts from (dpb.c:160-170) */
int32_t hl_amd_get_recon(hl_amd_encoder_t* encoder, uint8_t* y, uint8_t* u, uint8_t* v);

/* Time of the last encode call, in milliseconds, split by stage.
 * Per-picture calls: [0] quarter-pel planes kernel, [1] macroblock-decision
 * kernels (sum over the wavefront launches, re-runs included), [2]
 * deblocking kernels, [3] the frame's device timeline from planes to
 * deblock end (host validation gaps included).
 * Pipelined runs (hl_amd_encode_batch): [0] planes of the picture before
 * the run, [1] the pipelined kernel, [2] the copy of the run's records to
 * the host, [3] host slice writing (wall time).  Filled only when timing is
 * on. */
int32_t hl_amd_set_timing(hl_amd_encoder_t* encoder, int32_t enable);
int32_t hl_amd_get_timing(hl_amd_encoder_t* encoder, float* ms4);

/* number of row-start re-runs the last frame needed (rdo.Single_ctr
 * speculation) -- diagnostics */
int32_t hl_amd_last_reruns(hl_amd_encoder_t* encoder);

/* number of in-kernel rdo.Single_ctr walks (resolve_chain: a row start
 * read the counter while its value was still speculated) in the last
 * pipelined run -- diagnostics */
int32_t hl_amd_last_chain_walks(hl_amd_encoder_t* encoder);

/* Diagnostics: `iters` launches of the quarter-pel plane kernel on the
 * encoder's current reference picture; *ms = average ms per launch (the
 * HBM-bound kernel's own roofline line in bench.py).  No reference interface. */
int32_t hl_amd_bench_planes(hl_amd_encoder_t* encoder, int32_t iters, float* ms);

/* number of macroblock-decision kernel launches of the last frame */
int32_t hl_amd_last_mb_launches(hl_amd_encoder_t* encoder);

/* How the last encode call (hl_amd_encode*, or one base-layer chunk of
 * hl_amd_encode_layers_batch) ran -- diagnostics, no reference interface:
 * out5[0] pipelined runs launched, [1] pictures coded on the per-picture
 * wavefront path, [2] runs that fell back to it (re-encoded picture by
 * picture), [3] bounded waits that gave up, [4] in-kernel rdo.Single_ctr
 * walks.  A healthy call has [1] = [2] = [3] = 0. */
int32_t hl_amd_last_batch_stats(hl_amd_encoder_t* encoder, int32_t* out5);

/* Intra helper tasks (pipelined runs, on by default; also HL_AMD_HELPERS=0
 * at create): a P macroblock's intra fallback (rdo.c:1161-1167) is prepared
 * by a second workgroup beside the macroblock's inter search -- every
 * Intra16x16 mode's transform, quantisation, CAVLC statistics and
 * reconstruction, and the Intra4x4 decision under a guess of the live
 * TotalCoeffs that the macroblock verifies; and, in a run
 * of one picture (the per-frame path), a third workgroup searches the
 * macroblock's P8x8 partitionings from its MB-start live TotalCoeffs while
 * the macroblock searches the larger ones, proven by nC-class intervals
 * before the macroblock takes them (HL_AMD_FAM3=0 at create
 * turns that part off).  Results do not depend on it.  No reference
 * interface. */
int32_t hl_amd_set_intra_helpers(hl_amd_encoder_t* encoder, int32_t enable);

/* How the intra fallbacks of the last encode call ran -- diagnostics:
 * out3[0] P macroblocks that kept their helper's Intra4x4 decision, [1]
 * that rejected it (an nC class differed: decided again), [2] whose helper
 * no workgroup had claimed in time (the macroblock decided intra itself). */
int32_t hl_amd_last_helper_stats(hl_amd_encoder_t* encoder, int32_t* out3);

/* How the 8x8-family helpers of the last encode call ran -- diagnostics:
 * out2[0] P macroblocks that took their helper's P8x8 searches, [1] that
 * found them unproven for their entry state (searched again). */
int32_t hl_amd_last_fam3_stats(hl_amd_encoder_t* encoder, int32_t* out2);

/* per-phase shader-clock counters of the macroblock kernel; filled only by
 * the profiling build (make profile); out[2k] = cycles, out[2k+1] = calls
 * for k < 32, then out[64 + addr] = cycles of macroblock addr in the last
 * frame (n <= 64 + macroblocks).  The phase counters are cleared by the call. */
int32_t hl_amd_profile_counters(hl_amd_encoder_t* encoder, unsigned long long* out, int32_t n);

/* diagnostics: the macroblock records (syntax handed to the slice writer,
 * hartallo_amd/csrc/hl_types.h MbRecord) of picture k of the last encode
 * call, bytes = macroblocks * hl_amd_record_size(); INVALID_STATE when the
 * call did not keep them (a run re-encoded picture by picture) */
int32_t hl_amd_debug_records(hl_amd_encoder_t* encoder, int32_t k, void* out, size_t bytes);
int32_t hl_amd_record_size(void);

/* diagnostics: the rdo.Single_ctr chain records (hl_types.h MbChain, 20 bytes
 * per macroblock) and the reconstructed (deblocked) planes of picture k of
 * the last encode call */
int32_t hl_amd_debug_chain(hl_amd_encoder_t* encoder, int32_t k, void* out, size_t bytes);
int32_t hl_amd_debug_recon(hl_amd_encoder_t* encoder, int32_t k, uint8_t* y, uint8_t* u, uint8_t* v);

/* ---- Spatial SVC (Annex G) ----
 * hl_codec_add_layer (source/hl_codec.c:95-131): layers in increasing order,
 * the first one of the encoder's own size; each further layer twice the one
 * below (the reference accepts any power-of-two ratio, its encoder is only
 * exercised dyadic; other ratios return NOT_IMPLEMENTED).  At most 4 layers
 * (HL_ENCODER_MAX_LAYERS, OUTOFCAPACITY).  Call before the first frame. */
int32_t hl_amd_add_layer(hl_amd_encoder_t* encoder, int32_t width, int32_t height);

/* plugin encode() of a frame of the given size (hl_frame_video_t.data_width /
 * data_height[0]): with layers, the frame's size selects the layer
 * (hl_codec_264.c:470-483, NOT_FOUND otherwise) and the layers of an access
 * unit come in increasing order (INVALID_STATE otherwise).  Like the
 * reference, result.type has HDR whenever the header set grew (the first
 * frame of each layer; result.hdr then holds every SPS, subset SPS and PPS)
 * and DATA only with the access unit's last layer (result.data = prefix NAL,
 * base slice and enhancement slices, "00 00 01"-separated, no leading start
 * code; hl_codec_264.c:999-1017).  on_device: planes in HBM (else host).
 * Without layers this is hl_amd_encode / hl_amd_encode_device. */
int32_t hl_amd_encode_layer(hl_amd_encoder_t* encoder, int32_t width, int32_t height, const uint8_t* y, const uint8_t* u,
                            const uint8_t* v, int32_t on_device, hl_amd_result_t* result);

/* reconstructed (deblocked) picture of layer `layer` after its last frame */
int32_t hl_amd_get_layer_recon(hl_amd_encoder_t* encoder, int32_t layer, uint8_t* y, uint8_t* u, uint8_t* v);

/* enhancement-layer macroblocks coded so far whose reference-layer macroblock
 * was intra in a P picture: the reference's output there depends on its
 * uninitialised scratch memory (hartallo_amd/csrc/hl_svc.h), so they are
 * outside the bit-exact guarantee; 0 on every pinned workload */
int32_t hl_amd_svc_unpinned(hl_amd_encoder_t* encoder);

/* Layer-sharded coding (one process / GPU per layer).  An encoder with all
 * layers added codes only layers [first, last] (no reference interface: the
 * reference codes every layer in one hl_codec_t).  Per access unit the rank
 * coding the layer below `first` exports that layer's state -- picture
 * Y|U|V and macroblock objects, hl_amd_layer_state_bytes() bytes -- into a
 * device buffer (hl_amd_export_layer, after its last call of the access
 * unit), the buffer travels (RCCL over xGMI), and this encoder imports it
 * (hl_amd_import_layer) before coding `first`.  The DATA of the call for
 * `last` then holds only layers [first, last] ("00 00 01"-separated); the
 * access unit is the ranks' parts joined with "00 00 01" in layer order. */
int32_t hl_amd_set_layer_range(hl_amd_encoder_t* encoder, int32_t first, int32_t last);
size_t hl_amd_layer_state_bytes(hl_amd_encoder_t* encoder, int32_t layer);
int32_t hl_amd_export_layer(hl_amd_encoder_t* encoder, int32_t layer, void* dst_device);
int32_t hl_amd_import_layer(hl_amd_encoder_t* encoder, int32_t layer, const void* src_device);

/* n access units of every layer (planes in HBM; planes[(l * n + i) * 3 + c]
 * = plane c of layer l's frame of access unit i), as if by the
 * hl_amd_encode_layer calls for them: the base-layer pictures are coded
 * frame-pipelined (hl_amd_encode_batch), then every enhancement layer.
 * results[i] = access unit i: HDR with every header set those calls signal,
 * in order, and DATA; valid until the next call.  Needs every layer coded by
 * this encoder (no layer range).  No reference interface: a throughput entry
 * point like hl_amd_encode_batch.  A call that fails part-way leaves the
 * layers of its access units inconsistent: every later call then returns
 * HL_AMD_ERROR_INVALID_STATE, and destroying and re-creating the encoder is
 * the only reset. */
int32_t hl_amd_encode_layers_batch(hl_amd_encoder_t* encoder, int32_t n, int32_t layers, const uint8_t* const* planes,
                                   hl_amd_result_t* results);

/* ---- access units from the top layer's frame ----
 * No reference interface: the reference's caller scales every layer itself
 * (its test driver reads one file per layer, test_encoder.c:100-111).  Here
 * the caller hands over the top layer's frame only and the encoder derives
 * the lower layers' input on the GPU (k_pyramid, hartallo_amd/csrc/
 * hl_pyramid.h): layer l = the 2x2 box average (a + b + c + d + 2) >> 2 of
 * layer l + 1, every plane on its own, rounded at every level -- the filter
 * of hartallo_amd.synth.svc_clips, so a stream coded from the top clip alone
 * equals the one coded from svc_clips' layers.
 *
 * hl_amd_encode_au: one access unit.  The frame (host planes, or planes in
 * HBM with on_device) becomes the top layer's input, one k_pyramid launch on
 * the encoder's stream writes the input planes of the layers below, and the
 * layers are coded as by hl_amd_encode_layer(..., on_device = 1, ...) for
 * layer 0, 1, ... -- the GOP counter, idr_pic_id and every other rule are that
 * call's.  result folds those calls' results: HDR if any of them signalled
 * it, hdr then every header set they signalled, in order (what a caller of
 * the layer calls writes out: the reference's driver writes the header bytes
 * at each such call, test_encoder.c:220-236); DATA the access unit.
 * HL_AMD_ERROR_INVALID_STATE with fewer than 2 layers, with a layer range
 * other than all layers (hl_amd_set_layer_range), and between the
 * hl_amd_encode_layer calls of an unfinished access unit;
 * HL_AMD_ERROR_NOT_IMPLEMENTED under rate control (as hl_amd_encode_layer).
 * A refused call leaves the encoder as it was. */
int32_t hl_amd_encode_au(hl_amd_encoder_t* encoder, const uint8_t* y, const uint8_t* u, const uint8_t* v, int32_t on_device,
                         hl_amd_result_t* result);

/* n access units from n top-layer frames in HBM (top_planes[3 * i + c] =
 * plane c of access unit i's frame, 8-byte aligned): one k_pyramid launch
 * derives the lower layers' planes of all n frames into device buffers the
 * encoder owns, then the access units are coded by
 * hl_amd_encode_layers_batch: its results, its failure contract and its
 * refusals.  No reference interface. */
int32_t hl_amd_encode_aus_batch(hl_amd_encoder_t* encoder, int32_t n, const uint8_t* const* top_planes, hl_amd_result_t* results);

/* the input planes the last hl_amd_encode_au derived for `layer` (for the top
 * layer: the frame itself), copied to the host; after hl_amd_encode_aus_batch
 * those of its last frame.  A top frame handed over in HBM is read from the
 * caller's planes, which must still be there.  Valid until the next encode
 * call.
 * HL_AMD_ERROR_INVALID_STATE before the first such call.  For callers who
 * want the thumbnails, and for the tests.  No reference interface. */
int32_t hl_amd_get_layer_input(hl_amd_encoder_t* encoder, int32_t layer, uint8_t* y, uint8_t* u, uint8_t* v);

/* ---- access units of any display size, from frames in any format ----
 * No reference interface (like hl_amd_set_display_size and
 * hl_amd_encode_frame, whose counterparts for an encoder with layers these
 * are).
 *
 * hl_amd_set_au_display_size: the display size dw x dh of the TOP layer of an
 * encoder with L >= 2 layers (K = L - 1, top coded size W x H = the base size
 * shifted left by K).  Accepted: dw and dh multiples of 2 << K with
 * W - (16 << K) < dw <= W and H - (16 << K) < dh <= H, else
 * HL_AMD_ERROR_INVALID_PARAMETER; (W, H) means none.  Layer l then has the
 * display size (dw >> (K - l), dh >> (K - l)): even, the base layer crops less
 * than a macroblock, layer l up to (16 << l) - 2 samples -- whole macroblock
 * rows and columns that are coded and cropped, which H.264 allows.  1920x1080
 * in three layers: coded 1920x1088, 960x544, 480x272; 1280x720: coded
 * 1280x768, 640x384, 320x192.  SPS 0 carries the base layer's cropping as
 * hl_amd_set_display_size writes it, every subset SPS frame_cropping_flag = 1
 * with left 0, right (W_l - dw_l) / 2, top 0, bottom (H_l - dh_l) / 2 (escaped
 * like the SPS); every other field, level_idc, max_num_ref_frames and the SVC
 * extension included (extended_spatial_scalability_idc stays 0: inter-layer
 * prediction is between coded sizes), the PPSs and every slice NAL unit are
 * unchanged.  HL_AMD_ERROR_INVALID_STATE on an encoder without (all) its
 * layers, after the first picture and inside an access unit;
 * HL_AMD_ERROR_NOT_IMPLEMENTED together with a layer range other than all
 * layers (hl_amd_set_layer_range, in either order).  Works in either order
 * with hl_amd_set_max_ref_frame; hl_amd_add_layer after it returns
 * HL_AMD_ERROR_NOT_IMPLEMENTED.  Off by default: it changes no byte of a
 * stream coded without it.
 * Which call takes which size: hl_amd_encode_layer, hl_amd_encode_layers_batch,
 * hl_amd_encode_au and hl_amd_encode_aus_batch keep taking planes of the coded
 * sizes that the caller padded (the setting changes their headers and the
 * quality window only); hl_amd_encode_au_frame(s) take frames of the top
 * display size.  Quality (hl_amd_last_quality, hl_amd_debug_quality_mb) then
 * covers layer l's display rectangle. */
int32_t hl_amd_set_au_display_size(hl_amd_encoder_t* encoder, int32_t width, int32_t height);
/* the top layer's display size (its coded size when none was set) */
int32_t hl_amd_get_au_display_size(hl_amd_encoder_t* encoder, int32_t* width, int32_t* height);

/* Every header NAL unit ("00 00 01"-prefixed: SPS 0, the subset SPSs, the
 * PPSs) that an encoder created with these parameters (the base layer's width
 * and height, qp) and `layers` dyadic layers emits once every layer is coded,
 * after hl_amd_set_max_ref_frame(max_ref_frame) and
 * hl_amd_set_au_display_size(display_width, display_height) -- the top coded
 * size for no cropping.  A pure function (no device), the counterpart of
 * hl_amd_stream_headers.  Returns the bytes written, or 0 when a setting is
 * refused or the bytes do not fit in cap. */
size_t hl_amd_svc_stream_headers(const hl_amd_params_t* params, int32_t max_ref_frame, int32_t layers, int32_t display_width,
                                 int32_t display_height, uint8_t* out, size_t cap);

/* One access unit from one described frame (hl_amd_frame_t below), on the host
 * or in HBM, of the top display size (the top coded size when none is set):
 * k_ingest and, below the coded size, k_ingest_edge write the top layer's
 * coded planes -- the edge replication of the converted frame through clamped
 * coordinates, margins up to (16 << K) - 2; for RGB chroma still comes from the
 * source 2x2 block -- then everything is hl_amd_encode_au's on those planes:
 * k_pyramid derives every lower layer from the padded top picture, and the
 * result, the GOP counter and idr_pic_id are its own.  The matrix is
 * hl_amd_set_colour's; host frames are staged with a pitch rounded up to 4,
 * device planes and pitches are multiples of 4.  A dense I420 device frame of
 * the coded size is handed to hl_amd_encode_au untouched.  Every check comes
 * before anything is uploaded or launched and a refused call leaves the
 * encoder as it was: HL_AMD_ERROR_INVALID_STATE without layers, with a layer
 * range, inside an access unit of layer calls and on an encoder an earlier
 * GPU failure left unusable; HL_AMD_ERROR_NOT_IMPLEMENTED under rate control;
 * HL_AMD_ERROR_INVALID_PARAMETER for the frame (see hl_amd_encode_frame).  No
 * ctl: layers take no forced types. */
struct hl_amd_frame_s;
int32_t hl_amd_encode_au_frame(hl_amd_encoder_t* encoder, const struct hl_amd_frame_s* frame, hl_amd_result_t* result);

/* n access units from n described frames in HBM (a host frame:
 * HL_AMD_ERROR_INVALID_PARAMETER): one ingest launch per format present writes
 * n dense top frames into a buffer the encoder owns, then
 * hl_amd_encode_aus_batch codes them: its results, failure contract and
 * refusals. */
int32_t hl_amd_encode_au_frames(hl_amd_encoder_t* encoder, int32_t n, const struct hl_amd_frame_s* frames, hl_amd_result_t* results);

/* Diagnostics: `iters` launches of k_pyramid on the frame of the last
 * hl_amd_encode_au (the same planes into the same buffers); *ms = average ms
 * per launch.  HL_AMD_ERROR_INVALID_STATE without such a call.  No reference
 * interface. */
int32_t hl_amd_bench_pyramid(hl_amd_encoder_t* encoder, int32_t iters, float* ms);

/* Scene-cut detection.  No reference interface: the reference's picture types
 * come from gop_size and hl_frame_t.encoding alone, and nothing there looks
 * at the pictures.  With threshold 1..256 every input frame of an encode call
 * is compared on the GPU with the input frame before it (k_scene: per 16x16
 * luma macroblock intra = sum |p - mean| and inter = the smallest SAD over the
 * displacements of [-range, range]^2 that stay inside the picture; per frame
 * P = sum min(inter, intra), I = sum intra), and a frame with
 * hl_amd_scene_is_cut(P, I, threshold), at least min_gap pictures after the
 * last IDR of any cause and with encoding AUTO (or no ctl) is coded exactly as
 * if the caller had passed HL_AMD_ENCODING_INTRA for it: the stream is the
 * reference's for those hl_frame_t.encoding values.  HL_AMD_ENCODING_INTER is
 * the caller's veto.  The first frame of a stream, and the first after the
 * feature is switched on, have no previous frame and are never cuts.  Honoured
 * by hl_amd_encode, _device, _batch, _streams (every encoder its own setting
 * and state), their _ex forms and the look-ahead queue (analysed when the
 * queue is coded).  A refused or failed call leaves the detector's state as
 * it was.  With the feature on, device planes must be 4-byte aligned
 * (HL_AMD_ERROR_INVALID_PARAMETER).
 * threshold 0: off (the default; nothing is launched or allocated).
 * min_gap >= 1, range 0..16, threshold 0..256, else
 * HL_AMD_ERROR_INVALID_PARAMETER.  Between any two encode calls; while
 * look-ahead frames are queued HL_AMD_ERROR_INVALID_STATE; on an encoder with
 * layers HL_AMD_ERROR_NOT_IMPLEMENTED (layers take no forced types; adding a
 * layer switches the feature off). */
int32_t hl_amd_set_scenecut(hl_amd_encoder_t* encoder, int32_t threshold, int32_t min_gap, int32_t range);

/* The detector's rule, a pure function (no device): 1 when I > 0 and
 * 256 P >= threshold I, else 0; -1 for a threshold outside 1..256.  No
 * reference interface (the rule is this project's). */
int32_t hl_amd_scene_is_cut(uint64_t P, uint64_t I, int32_t threshold);

/* Picture k of the last encode call (with look-ahead: the call that coded the
 * queue): out4 = P, I, 1 if the picture was analysed, 1 if the detector turned
 * it into an IDR.  HL_AMD_ERROR_INVALID_STATE when that call ran with the
 * feature off.  No reference interface (nothing there to report). */
int32_t hl_amd_last_scene_stats(hl_amd_encoder_t* encoder, int32_t k, uint64_t out4[4]);

/* Diagnostics: inter and intra of every macroblock (mbs = the picture's
 * macroblock count) of picture k of the last encode call;
 * HL_AMD_ERROR_INVALID_STATE for a picture that was not analysed.  No
 * reference interface (the tests' handle on k_scene). */
int32_t hl_amd_debug_scene_mb(hl_amd_encoder_t* encoder, int32_t k, uint32_t* inter, uint32_t* intra, size_t mbs);

/* Diagnostics: `iters` times the analysis launch of the last encode call (the
 * same frames, which must still be there, into the same arrays); *ms = average
 * ms per launch.  HL_AMD_ERROR_INVALID_STATE without such a launch.  No
 * reference interface (like hl_amd_bench_pyramid). */
int32_t hl_amd_bench_scene(hl_amd_encoder_t* encoder, int32_t iters, float* ms);

/* Per-picture quality: PSNR and SSIM sums of every coded picture against the
 * planes it was coded from, computed on the GPU while both are resident
 * (k_quality, hl_quality.h).  No reference interface: the reference has
 * nothing that measures a coded picture.  It changes no byte of any stream.
 * Integers only, exact in any order.  Per plane c (0 Y, 1 U, 2 V), with a =
 * source and b = deblocked reconstruction:
 *   sse[c]      = sum (a - b)^2                  samples[c] = the plane's W H
 *   ssim_q30[c] = sum over the plane's 8x8 windows (stride 4: (W/4 - 1)
 *                 (H/4 - 1) = windows[c] of them) of floor(num 2^30 / den),
 *     S1 = sum a, S2 = sum b, SS = sum (a^2 + b^2), S12 = sum a b of the window,
 *     num = (2 S1 S2 + 416)(2 (64 S12 - S1 S2) + 235963),
 *     den = (S1^2 + S2^2 + 416)(64 SS - S1^2 - S2^2 + 235963).
 * hl_amd_psnr_db and hl_amd_ssim_mean turn them into the usual figures.
 * With a display size (hl_amd_set_display_size) "the plane" above is the
 * plane's display rectangle, w x h = dw x dh of luma and dw/2 x dh/2 of chroma
 * (odd sizes and sizes that are no multiples of 4 included): samples[c] = w h,
 * sse[c] runs over its samples, ssim_q30[c] over the 8x8 windows at stride 4
 * that lie wholly inside it, windows[c] = max(0, w/4 - 1) max(0, h/4 - 1)
 * (integer divisions), and hl_amd_debug_quality_mb gives the SSE of each
 * macroblock's display part.  Without one every result is what it was. */
typedef struct hl_amd_quality_s {
    uint64_t sse[3], samples[3];
    int64_t ssim_q30[3];
    uint64_t windows[3];
} hl_amd_quality_t;

/* enable 0: off (the default; nothing is launched or allocated), else on.
 * Honoured by hl_amd_encode, _device, _batch, _streams (every encoder its own
 * setting), their _ex forms, the look-ahead queue (measured when the queue is
 * coded), rate-controlled encoders and, on encoders with layers, every layer
 * this encoder codes (hl_amd_encode_layer, _au: k = 0; hl_amd_encode_layers_batch,
 * hl_amd_encode_aus_batch: k = the access unit).  While the feature is on,
 * device planes must be 8-byte aligned: a call with another plane returns
 * HL_AMD_ERROR_INVALID_PARAMETER before anything is coded.  Between any two
 * encode calls; while look-ahead frames are queued
 * HL_AMD_ERROR_INVALID_STATE.  No reference interface (see above). */
int32_t hl_amd_set_quality(hl_amd_encoder_t* encoder, int32_t enable);

/* Picture k of layer `layer` (0 on encoders without layers) of the last
 * encode call (with look-ahead: the call that coded the queue).
 * HL_AMD_ERROR_INVALID_STATE when that picture or layer was not measured: the
 * feature was off, the layer is coded elsewhere (hl_amd_set_layer_range), or
 * the last call was refused or failed.  No reference interface (see above). */
int32_t hl_amd_last_quality(hl_amd_encoder_t* encoder, int32_t layer, int32_t k, hl_amd_quality_t* out);

/* Diagnostics: sum (a - b)^2 of every 16x16 luma macroblock (mbs = the
 * layer's macroblock count) of that picture; the same refusals.  No
 * reference interface (the tests' handle on k_quality). */
int32_t hl_amd_debug_quality_mb(hl_amd_encoder_t* encoder, int32_t layer, int32_t k, uint32_t* sse_y, size_t mbs);

/* Diagnostics: `iters` times the last measurement launch of the AVC path (the
 * same planes, which must still be there, into the same sums, which are
 * unusable afterwards: hl_amd_last_quality returns HL_AMD_ERROR_INVALID_STATE
 * until the next encode call); *ms = average ms per launch.
 * HL_AMD_ERROR_INVALID_STATE without such a launch.  No reference interface
 * (like hl_amd_bench_scene). */
int32_t hl_amd_bench_quality(hl_amd_encoder_t* encoder, int32_t iters, float* ms);

/* Pure functions (no device): 10 log10(255^2 samples / sse), +infinity for
 * sse = 0, NaN for samples = 0; and q30 / 2^30 / windows, NaN for windows = 0
 * or |q30| > windows 2^30.  No reference interface (see above). */
double hl_amd_psnr_db(uint64_t sse, uint64_t samples);
double hl_amd_ssim_mean(int64_t q30, uint64_t windows);

/* ---- frames that are not dense planar I420 ----
 * No reference interface: hl_frame_video_t (hl_frame.h:278-291) has neither a
 * pitch nor a format.  A frame is described by its format, its planes and the
 * bytes between their rows; the picture size is the encoder's.  Row bytes per
 * plane: I420 W, W/2, W/2; NV12 W, W; RGB24 3W; RGBA32 4W (byte 3 of a sample
 * is ignored); RGBP W, W, W.  Only the bytes [plane + r pitch, plane + r pitch
 * + row bytes) of a row are ever read: a plane's last row needs no padding
 * after it (a cropped view of a larger image works).
 * One GPU kernel (k_ingest, hartallo_amd/csrc/hl_ingest.h) turns the frame
 * into the dense I420 planes the unchanged coding path takes:
 *   - I420 and NV12 are copied (de-pitched, NV12's chroma de-interleaved);
 *   - RGB is converted with integers only,
 *       Y = (yr R + yg G + yb B + (off << 16) + (1 << 15)) >> 16 per sample,
 *       U = min(255, (ur SR + ug SG + ub SB + (128 << 18) + (1 << 17)) >> 18)
 *     and V likewise per 2x2 block from the sums SR, SG, SB of its four
 *     samples (chroma sited at the block's centre, rounded once).  Tables
 *     (y | u | v | off), derived in hl_ingest.h from Kr, Kb and the range:
 *       601 limited (16829 33039 6416 | -9714 -19070 28784 | 28784 -24103 -4681 | 16)
 *       601 full    (19595 38470 7471 | -11058 -21710 32768 | 32768 -27439 -5329 | 0)
 *       709 limited (11966 40254 4064 | -6596 -22188 28784 | 28784 -26145 -2639 | 16)
 *       709 full    (13933 46871 4732 | -7509 -25259 32768 | 32768 -29763 -3005 | 0)
 *     Grey input gives U = V = 128 exactly.  The default is BT.601 limited.
 *     The stream carries no VUI colour description (the reference writes
 *     none): which matrix was used travels out of band.
 * The coded size stays a multiple of 16.  With a display size
 * (hl_amd_set_display_size) W and H above are the display size dw x dh: the
 * frames have its rows and row bytes, and a second kernel (k_ingest_edge, one
 * lane per tile of 16 x 2 samples that is not wholly inside the frame: at most
 * one tile column and seven tile rows) pads the planes to the coded size by
 * the edge replication defined there, loading single bytes by clamped
 * coordinate.  Spatial layers are not served (HL_AMD_ERROR_NOT_IMPLEMENTED). */
enum {
    HL_AMD_FORMAT_I420 = 0,
    HL_AMD_FORMAT_NV12,
    HL_AMD_FORMAT_RGB24,
    HL_AMD_FORMAT_RGBA32,
    HL_AMD_FORMAT_RGBP
};
enum { HL_AMD_MATRIX_BT601 = 0, HL_AMD_MATRIX_BT709 };
enum { HL_AMD_RANGE_LIMITED = 0, HL_AMD_RANGE_FULL };

typedef struct hl_amd_frame_s {
    int32_t format, on_device; /* HL_AMD_FORMAT_*; on_device: planes in HBM, else host */
    const uint8_t* plane[3];   /* I420: Y,U,V  NV12: Y,UV  RGB24/RGBA32: one  RGBP: R,G,B */
    int64_t pitch[3];          /* bytes between rows; 0 = dense (row bytes) */
} hl_amd_frame_t;

/* Validation of the frame calls below covers every frame of a call and
 * happens before anything is uploaded, converted or queued; a refused call
 * leaves the encoder as it was and the next call continues the stream.
 * HL_AMD_ERROR_INVALID_PARAMETER: an unknown format; a null plane the format
 * needs; a pitch that is negative, or non-zero and below row bytes; a device
 * plane or pitch that is no multiple of 4 (k_ingest loads 4-byte words; a
 * pitch of 0 counts as the row bytes, so a dense device frame of a display
 * width like 34 is refused, while any even width works from the host, whose
 * rows are staged with a pitch rounded up to a multiple of 4).
 * HL_AMD_ERROR_NOT_IMPLEMENTED: an encoder with spatial layers.  The ctl is
 * checked as in the _ex calls.  HL_AMD_ERROR_INVALID_STATE: an encoder that
 * an earlier GPU failure has left unusable.
 * A dense I420 frame in device memory (every pitch 0 or row bytes) of the
 * coded size (no display size below it is set) is
 * forwarded untouched -- no copy, no kernel: it is hl_amd_encode_device_ex's
 * frame, the 4-byte rule does not apply to it, and the alignment rules of
 * scene-cut detection and quality apply to the caller's planes as there.
 * (With look-ahead on, hl_amd_encode_frame copies such a frame into the queue
 * as hl_amd_encode_ex does, and no alignment rule applies to it.) */

/* The matrix and range RGB frames are converted with from now on
 * (HL_AMD_MATRIX_*, HL_AMD_RANGE_*; anything else
 * HL_AMD_ERROR_INVALID_PARAMETER).  Between any two encode calls; while
 * look-ahead frames are queued HL_AMD_ERROR_INVALID_STATE.  No reference
 * interface (see above). */
int32_t hl_amd_set_colour(hl_amd_encoder_t* encoder, int32_t matrix, int32_t range);

/* One frame: hl_amd_encode_ex / hl_amd_encode_device_ex for a described
 * frame.  A host frame is uploaded row by row (padding is not read) into a
 * staging buffer the encoder owns, a device frame is read in place; one
 * k_ingest launch on the encoder's stream writes the encoder's input planes
 * (with look-ahead: the queue's next slot), and the frame then goes through
 * exactly what those calls run: the result, the GOP counter, rate control,
 * scene cuts and quality (source = the converted planes) are theirs.  No
 * reference interface (see above). */
int32_t hl_amd_encode_frame(hl_amd_encoder_t* encoder, const hl_amd_frame_t* frame, const hl_amd_frame_ctl_t* ctl,
                            hl_amd_result_t* result);

/* n frames in device memory (a host frame: HL_AMD_ERROR_INVALID_PARAMETER):
 * hl_amd_encode_batch_ex for described frames.  Every frame that is not
 * forwarded is converted first, into a buffer of dense I420 frames the encoder
 * owns -- one k_ingest launch per format the call holds -- and the n frames
 * are then coded as by hl_amd_encode_batch_ex: its results, its split into
 * runs and its failure contract.  HL_AMD_ERROR_INVALID_STATE while look-ahead
 * frames are queued.  No reference interface (see above). */
int32_t hl_amd_encode_frames(hl_amd_encoder_t* encoder, int32_t n, const hl_amd_frame_t* frames, const hl_amd_frame_ctl_t* ctl,
                             hl_amd_result_t* results);

/* The planes picture k of the last hl_amd_encode_frame / hl_amd_encode_frames
 * call was coded from, copied to the host: what was encoded.
 * HL_AMD_ERROR_INVALID_STATE before such a call, after a refused or failed
 * one, after any other encode call, for a forwarded frame (its planes are the
 * caller's) and with look-ahead on.  No reference interface (see above). */
int32_t hl_amd_get_input(hl_amd_encoder_t* encoder, int32_t k, uint8_t* y, uint8_t* u, uint8_t* v);

/* Diagnostics: `iters` times the k_ingest launch(es) of the last frame call
 * (the same frames, which must still be there, into the same planes); *ms =
 * average ms per repetition.  HL_AMD_ERROR_INVALID_STATE when that call
 * launched nothing (every frame forwarded) or did not succeed.  No reference
 * interface (like hl_amd_bench_pyramid). */
int32_t hl_amd_bench_ingest(hl_amd_encoder_t* encoder, int32_t iters, float* ms);

/* ---- frames larger than the picture ----
 * No reference interface: the reference has no scaler (test_encoder.c:100-111
 * reads one pre-scaled file per layer).  With a source size sw x sh the frames
 * of hl_amd_encode_frame / hl_amd_encode_frames have that size and are scaled
 * on the GPU to the display size dw x dh (the coded size unless one was set)
 * by an area filter defined in integers (hartallo_amd/csrc/hl_scale.h).  Per
 * axis, with a source length s and a destination length d, d <= s <= 8 d:
 * g = gcd(s, d), sr = s / g, dr = d / g; output sample j covers
 * [j sr, (j + 1) sr), source sample i covers [i dr, (i + 1) dr), and
 *   w(j, i) = max(0, min((j + 1) sr, (i + 1) dr) - max(j sr, i dr));
 * the taps of j are i = floor(j sr / dr) .. floor(((j + 1) sr - 1) / dr), at
 * most ceil(sr / dr) + 1 <= 9, every weight positive, their sum sr.  A plane,
 * with D = srw srh:
 *   out(x, y) = floor((sum_k sum_i wv(y, k) wh(x, i) p(k, i) + (D >> 1)) / D):
 * separable, unrounded, rounded once, half up; every quantity fits 32
 * unsigned bits.  Luma goes sw x sh -> dw x dh; U and V go sw/2 x sh/2 ->
 * dw/2 x dh/2 by the same formulas (chroma stays centre-sited, as in the
 * ingest).  Beyond the display size the coded planes take
 * out(min(x, dw - 1), min(y, dh - 1)): the display size's edge replication.
 * 2:1 on both axes is the 2x2 box of k_pyramid (the SVC layers' filter) bit
 * for bit; 4:1 is NOT that box applied twice, which rounds at each stage (on a
 * 96x64 noise plane 77 of the 384 samples differ).
 * Data path: the frame goes through k_ingest at the source size -- formats,
 * colour tables, the 4-byte rule of device planes and the read contract hold
 * with W, H = sw, sh -- into an intermediate I420 buffer the encoder owns, and
 * k_scale writes the encoder's input planes (the look-ahead slot, the frame's
 * planes of hl_amd_encode_frames) from it.  Nothing is forwarded.  Scene cuts,
 * quality (source = the scaled planes), rate control, the GOP counter and the
 * look-ahead see planes of the coded size; hl_amd_get_input returns the scaled,
 * padded planes: what was encoded.  The plain entry points (hl_amd_encode,
 * _device, _batch, _streams, the _ex forms, hl_amd_encode_au*) keep taking
 * planes of the coded size. */

/* The size of the frames from now on: even, dw <= width <= min(8 dw, 4096),
 * dh <= height <= min(8 dh, 4096), else HL_AMD_ERROR_INVALID_PARAMETER;
 * (dw, dh) turns scaling off, and the path is then the one without this call,
 * forwarding of dense I420 device frames included.  Between any two encode
 * calls (a source may change its resolution mid-stream), like
 * hl_amd_set_colour; HL_AMD_ERROR_INVALID_STATE while look-ahead frames are
 * queued; HL_AMD_ERROR_NOT_IMPLEMENTED on an encoder with spatial layers, and
 * from hl_amd_add_layer once a source size is set.  Set the display size
 * first: hl_amd_set_display_size returns HL_AMD_ERROR_INVALID_STATE while a
 * source size is set.  No reference interface (see above). */
int32_t hl_amd_set_source_size(hl_amd_encoder_t* encoder, int32_t width, int32_t height);

/* The size of the frame calls' frames: the source size, else the display
 * size.  No reference interface (see above). */
int32_t hl_amd_get_source_size(hl_amd_encoder_t* encoder, int32_t* width, int32_t* height);

/* The taps of output sample j of the axis s -> d (a pure function, no device,
 * like hl_amd_stream_headers): *first = the first source sample, weights[0 ..
 * count) its and its successors' weights; returns the count (1..9), or 0 for
 * what it refuses: s < d, s > 8 d, s > 4096, d <= 0, j outside [0, d), cap
 * below the count, a null pointer.  s and d may be odd (a chroma axis is).
 * No reference interface (see above). */
int32_t hl_amd_scale_taps(int32_t s, int32_t d, int32_t j, int32_t* first, uint32_t* weights, int32_t cap);

/* Diagnostics: `iters` times the k_scale launch(es) of the last frame call
 * (the same intermediate planes into the same planes); *ms = average ms per
 * repetition.  hl_amd_bench_ingest keeps repeating the ingest launches only.
 * HL_AMD_ERROR_INVALID_STATE when that call scaled nothing or did not
 * succeed.  No reference interface (like hl_amd_bench_ingest). */
int32_t hl_amd_bench_scale(hl_amd_encoder_t* encoder, int32_t iters, float* ms);

/* ---- a rendition ladder from one source ----
 * No reference interface: the reference has no scaler (see above).  `count`
 * encoders (1 to 8, distinct, on one device; the "rungs") are fed from the
 * same frame(s) of one common source size in one call: the frame(s) go ONCE
 * through the staging and k_ingest at the source size into encoders[0]'s
 * intermediate buffer, one k_scale_fan launch (hartallo_amd/csrc/hl_ladder.h;
 * several when frames x count exceed a grid dimension) writes every rung's
 * coded planes with the area filter above, and the rungs are then coded one
 * after another in the order of `encoders`.  Every rung is the direct area
 * filter of the source, never a cascade of another rung.
 * Contract: the results of rung r are exactly those of hl_amd_encode_frame
 * (hl_amd_encode_frames) on encoders[r] alone with the same frame(s) and its
 * own ctl: its own stream bytes, GOP counter and idr_pic_id, rate control,
 * scene cuts and quality, split into runs and failure contract.  Nothing is
 * forwarded: hl_amd_get_input(encoders[r], k, ...) returns rung r's scaled,
 * padded planes for every rung, an identity rung included.
 * Checked for every encoder, frame and ctl before anything is uploaded,
 * converted or launched (a refused call leaves every stream as it was):
 *   - count outside 1..8, a null or repeated encoder, encoders on different
 *     devices: HL_AMD_ERROR_INVALID_PARAMETER;
 *   - an encoder with spatial layers: HL_AMD_ERROR_NOT_IMPLEMENTED;
 *   - hl_amd_get_source_size must return the same (sw, sh) for every encoder
 *     (an encoder without a source size whose display size is (sw, sh) is an
 *     identity rung: the same filter with s = d), and every encoder must have
 *     the same hl_amd_set_colour setting (the conversion happens once), else
 *     HL_AMD_ERROR_INVALID_PARAMETER;
 *   - the frames as in the per-encoder calls, at the source size: the 4-byte
 *     rule of device planes always applies; host frames are taken by the
 *     single-frame call only;
 *   - frames queued by the look-ahead on any encoder, and for the single-frame
 *     call look-ahead on at all: HL_AMD_ERROR_INVALID_STATE;
 *   - ctl (null, or ctl[r * n + i] for frame i of rung r) as in the
 *     per-encoder calls, against rung r's size;
 *   - a broken encoder: HL_AMD_ERROR_INVALID_STATE.
 * If coding rung r fails after the checks, the rungs before it have committed
 * and keep their results, r follows its own call's failure contract, the
 * later rungs are untouched with their results zeroed, and r's error is
 * returned.  results[r * n + i]: frame i of rung r, valid until the next call
 * on encoders[r].  Left out: look-ahead ladders, rungs coded concurrently or
 * in one shared run, rungs with spatial layers, upscaling rungs, per-rung
 * colour settings. */
int32_t hl_amd_encode_ladder_frame(hl_amd_encoder_t* const* encoders, int32_t count, const hl_amd_frame_t* frame,
                                   const hl_amd_frame_ctl_t* ctl, hl_amd_result_t* results);
int32_t hl_amd_encode_ladder_frames(hl_amd_encoder_t* const* encoders, int32_t count, int32_t n, const hl_amd_frame_t* frames,
                                    const hl_amd_frame_ctl_t* ctl, hl_amd_result_t* results);

/* Diagnostics: `iters` times the k_scale_fan launch(es) of the last ladder
 * call, whose first encoder this is (the same intermediate planes into every
 * rung's planes; no other call on any of its encoders since); *ms = average
 * ms per repetition.  HL_AMD_ERROR_INVALID_STATE otherwise.  No reference
 * interface (like hl_amd_bench_scale). */
int32_t hl_amd_bench_ladder(hl_amd_encoder_t* encoder0, int32_t iters, float* ms);

/* device time (ms) of the enhancement layers of the last access unit (with
 * hl_amd_set_timing on) */
float hl_amd_svc_layer_ms(hl_amd_encoder_t* encoder);

const char* hl_amd_version(void);

#ifdef __cplusplus
}
#endif

#endif
