/*
 * ref_sched_harness.c -- TEST INFRASTRUCTURE.  oracle/ref_harness.c's job
 * (the *reference* encoder of oracle/_ref/libhl.a driven through its public
 * API like source/test_encoder.c:135-146) plus a per-frame schedule: the
 * caller sets hl_frame_t.encoding (hl_frame.h:38-39) and changes hl_codec_t
 * settings between hl_codec_encode calls, as a real-time application does.
 *
 * usage: ref_enc_sched W H N qp me_range deblock gop early_term in.yuv out_prefix TYPES CHANGES
 *   TYPES    one letter per frame, frames beyond its end are A ("-": all A):
 *            A = HL_VIDEO_ENCODING_TYPE_AUTO, I = _INTRA, P = _INTER,
 *            R = _RAW, L = _LOSSLESS
 *   CHANGES  "frame:key=value" items separated by ';' ("-": none), applied to
 *            the hl_codec_t right before that frame's call; keys me_range,
 *            deblock (deblock_flag), early_term (me_early_term_flag), gop
 *            (gop_size), qp
 * rate control from the environment as oracle/ref_harness.c:
 *   HL_REF_RC_BITRATE, HL_REF_RC_BASICUNIT, HL_REF_RC_QP_MIN, HL_REF_RC_QP_MAX
 * writes <prefix>.264 (Annex-B, as test_encoder.c:220-236), <prefix>.rec.yuv
 * (the reconstructed picture after every frame) and <prefix>.idx (the byte
 * offset where each frame's output ends).  A failing call prints
 * "encode err <code> at frame <f>" and exits with status 4.
 */
#include <hartallo/hl_api.h>
#include <hartallo/hl_frame.h>
#include <hartallo/hl_codec.h>
#include <hartallo/hl_object.h>
#include <hartallo/hl_debug.h>
#include <hartallo/hl_cpu.h>
#include <hartallo/h264/hl_codec_264.h>
#include <hartallo/h264/hl_codec_264_layer.h>
#include <hartallo/h264/hl_codec_264_dpb.h>
#include <hartallo/h264/hl_codec_264_pict.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sched.h"

int main(int argc, char** argv)
{
    if (argc < 13) {
        fprintf(stderr, "usage: %s W H N qp me_range deblock gop early_term in.yuv out_prefix TYPES CHANGES\n", argv[0]);
        return 1;
    }
    int W = atoi(argv[1]), H = atoi(argv[2]), N = atoi(argv[3]), qp = atoi(argv[4]);
    int mer = atoi(argv[5]), db = atoi(argv[6]), gop = atoi(argv[7]), et = atoi(argv[8]);
    const char* in = argv[9];
    const char* pre = argv[10];
    const char* types = argv[11];
    const char* changes = argv[12];
    char path[1024];

    hl_debug_set_level(HL_DEBUG_LEVEL_ERROR);
    hl_engine_set_cpu_flags(kCpuFlagAll);
    if (hl_engine_init()) return 2;

    const struct hl_codec_plugin_def_s* pl = 0;
    struct hl_codec_s* c = 0;
    struct hl_codec_result_s* r = 0;
    hl_frame_video_t* f = 0;
    hl_codec_plugin_find(HL_CODEC_TYPE_H264, &pl);
    hl_codec_create(pl, &c);
    hl_codec_result_create(&r);
    hl_frame_video_create(&f);
    c->gop_size = gop; c->me_range = mer; c->qp = qp; c->fps.num = 1; c->fps.den = 15;
    c->rc_bitrate = -1; c->deblock_flag = db; c->threads_count = 1; c->max_ref_frame = 1;
    c->distortion_mesure_type = HL_VIDEO_DISTORTION_MESURE_TYPE_SAD;
    c->me_type = (HL_VIDEO_ME_TYPE_INTEGER | HL_VIDEO_ME_TYPE_HALF | HL_VIDEO_ME_TYPE_QUATER);
    c->me_part_types = HL_VIDEO_ME_PART_TYPE_ALL;
    c->me_subpart_types = HL_VIDEO_ME_SUBPART_TYPE_ALL;
    c->me_early_term_flag = et;
    if (getenv("HL_REF_RC_BITRATE")) c->rc_bitrate = atoi(getenv("HL_REF_RC_BITRATE"));
    if (getenv("HL_REF_RC_BASICUNIT")) c->rc_basicunit = atoi(getenv("HL_REF_RC_BASICUNIT"));
    if (getenv("HL_REF_RC_QP_MIN")) c->rc_qp_min = atoi(getenv("HL_REF_RC_QP_MIN"));
    if (getenv("HL_REF_RC_QP_MAX")) c->rc_qp_max = atoi(getenv("HL_REF_RC_QP_MAX"));

    size_t fs = (size_t)W * H * 3 / 2;
    uint8_t* buf = (uint8_t*)malloc(fs);
    FILE* fi = fopen(in, "rb");
    if (!fi) { fprintf(stderr, "cannot open %s\n", in); return 3; }
    snprintf(path, sizeof(path), "%s.264", pre);
    FILE* fo = fopen(path, "wb");
    snprintf(path, sizeof(path), "%s.rec.yuv", pre);
    FILE* frec = fopen(path, "wb");
    snprintf(path, sizeof(path), "%s.idx", pre);
    FILE* fidx = fopen(path, "wb");
    static const uint8_t scp[3] = { 0, 0, 1 };
    int n = 0;
    while (n < N && fread(buf, 1, fs, fi) == fs) {
        if (sched_apply(changes, n, c)) return 1;
        hl_frame_video_fill(f, HL_VIDEO_CHROMA_YUV420, W, H, buf, fs);
        f->encoding = sched_type(types, n);
        int e = hl_codec_encode(c, (hl_frame_t*)f, r);
        if (e) { fprintf(stderr, "encode err %d at frame %d\n", e, n); return 4; }
        if (r->type & HL_CODEC_RESULT_TYPE_HDR) fwrite(c->hdr_bytes, 1, c->hdr_bytes_count, fo);
        if (r->type & HL_CODEC_RESULT_TYPE_DATA) { fwrite(scp, 1, 3, fo); fwrite(r->data_ptr, 1, r->data_size, fo); }
        fprintf(fidx, "%ld\n", ftell(fo));
        hl_codec_264_t* p264 = (hl_codec_264_t*)c;
        hl_codec_264_layer_t* L = p264->layers.pc_active;
        const hl_codec_264_pict_t* pict = L->pc_fs_curr->p_pict;
        fwrite(pict->pc_data_y, 1, (size_t)W * H, frec);
        fwrite(pict->pc_data_u, 1, (size_t)W * H / 4, frec);
        fwrite(pict->pc_data_v, 1, (size_t)W * H / 4, frec);
        n++;
    }
    fclose(fo);
    fclose(frec);
    fclose(fidx);
    printf("{\"frames\": %d}\n", n);
    return 0;
}
