/*
 * drop_in_sched_harness.c -- TEST INFRASTRUCTURE.  ref_sched_harness.c's
 * calls through the installed gfx950 plugin (integration/
 * hl_codec_264_gfx950.c, as oracle/drop_in_harness.c installs it): the
 * per-frame schedule (sched.h) sets hl_frame_t.encoding and changes the
 * hl_codec_t settings between hl_codec_encode calls, and every frame is
 * coded by libhartallo_amd.so on the GPU.
 *
 * usage: drop_in_sched W H N qp me_range deblock gop early_term in.yuv out.264 TYPES CHANGES
 *        drop_in_sched svc L W0 H0 N qp me_range deblock gop early_term out.264 TYPES CHANGES in0.yuv .. in{L-1}.yuv
 *   (svc: hl_codec_add_layer per layer, one hl_codec_encode per layer and
 *   frame, base first; the schedule applies to every layer's call of a frame)
 * rate control and the plugin's look-ahead (HL_AMD_LOOKAHEAD) from the
 * environment as oracle/drop_in_harness.c.  A failing call prints
 * "encode err <code> (<HL_ERROR_T name>) at frame <f>" and exits with status 6.
 */
#include <hartallo/hl_api.h>
#include <hartallo/hl_codec.h>
#include <hartallo/hl_cpu.h>
#include <hartallo/hl_debug.h>
#include <hartallo/hl_frame.h>
#include <hartallo/hl_object.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sched.h"

extern const hl_codec_plugin_def_t hl_codec_264_gfx950_plugin_def_s;
HL_ERROR_T hl_codec_264_gfx950_install(void);
HL_ERROR_T hl_codec_264_gfx950_flush(hl_codec_t* codec, hl_codec_result_t* result);

static const char* err_name(int e)
{
    switch (e) {
    case HL_ERROR_INVALID_PARAMETER: return "HL_ERROR_INVALID_PARAMETER";
    case HL_ERROR_INVALID_STATE: return "HL_ERROR_INVALID_STATE";
    case HL_ERROR_NOT_IMPLEMENTED: return "HL_ERROR_NOT_IMPLEMENTED";
    case HL_ERROR_TOOSHORT: return "HL_ERROR_TOOSHORT";
    default: return "HL_ERROR";
    }
}

static void put(const hl_codec_t* c, const hl_codec_result_t* r, FILE* fo)
{
    static const uint8_t scp[3] = {0, 0, 1};
    if (r->type & HL_CODEC_RESULT_TYPE_HDR) fwrite(c->hdr_bytes, 1, c->hdr_bytes_count, fo);
    if (r->type & HL_CODEC_RESULT_TYPE_DATA) {
        fwrite(scp, 1, 3, fo);
        fwrite(r->data_ptr, 1, r->data_size, fo);
    }
}

int main(int argc, char** argv)
{
    const int svc = argc > 1 && !strcmp(argv[1], "svc");
    char** a = svc ? argv + 2 : argv;
    const int need = svc ? 15 : 13;
    if (argc < need) {
        fprintf(stderr, "usage: %s W H N qp me_range deblock gop early_term in.yuv out.264 TYPES CHANGES\n"
                        "       %s svc L W0 H0 N qp me_range deblock gop early_term out.264 TYPES CHANGES in0.yuv ..\n", argv[0], argv[0]);
        return 1;
    }
    const int L = svc ? atoi(argv[2]) : 1;
    int W = atoi(a[1]), H = atoi(a[2]), N = atoi(a[3]), qp = atoi(a[4]);
    int mer = atoi(a[5]), db = atoi(a[6]), gop = atoi(a[7]), et = atoi(a[8]);
    const char* out = svc ? a[9] : a[10];
    const char* types = svc ? a[10] : a[11];
    const char* changes = svc ? a[11] : a[12];
    if (L < 1 || L > 4 || (svc && argc < 14 + L)) return 1;
    hl_debug_set_level(HL_DEBUG_LEVEL_ERROR);
    if (hl_engine_init()) return 2;
    if (hl_codec_264_gfx950_install()) return 3;
    const struct hl_codec_plugin_def_s* pl = 0;
    struct hl_codec_s* c = 0;
    struct hl_codec_result_s* r = 0;
    hl_frame_video_t* f = 0;
    if (hl_codec_plugin_find(svc ? HL_CODEC_TYPE_H264_SVC : HL_CODEC_TYPE_H264, &pl) || pl != &hl_codec_264_gfx950_plugin_def_s) {
        fprintf(stderr, "the gfx950 plugin is not the one hl_codec_plugin_find returns\n");
        return 4;
    }
    hl_codec_create(pl, &c);
    hl_codec_result_create(&r);
    hl_frame_video_create(&f);
    c->gop_size = gop; c->me_range = mer; c->qp = qp; c->fps.num = 1; c->fps.den = 15;
    c->rc_bitrate = -1; c->deblock_flag = db; c->threads_count = 1; c->max_ref_frame = 1;
    c->distortion_mesure_type = HL_VIDEO_DISTORTION_MESURE_TYPE_SAD;
    c->me_early_term_flag = et;
    if (getenv("HL_REF_RC_BITRATE")) c->rc_bitrate = atoi(getenv("HL_REF_RC_BITRATE"));
    if (getenv("HL_REF_RC_BASICUNIT")) c->rc_basicunit = atoi(getenv("HL_REF_RC_BASICUNIT"));
    if (getenv("HL_REF_RC_QP_MIN")) c->rc_qp_min = atoi(getenv("HL_REF_RC_QP_MIN"));
    if (getenv("HL_REF_RC_QP_MAX")) c->rc_qp_max = atoi(getenv("HL_REF_RC_QP_MAX"));
    FILE* fi[4] = {0};
    uint8_t* buf[4] = {0};
    size_t fs[4];
    for (int l = 0; l < L; ++l) {
        if (svc && hl_codec_add_layer(c, (uint32_t)(W << l), (uint32_t)(H << l), 0, 0)) return 5;
        fs[l] = (size_t)(W << l) * (H << l) * 3 / 2;
        buf[l] = (uint8_t*)malloc(fs[l]);
        if (!(fi[l] = fopen(svc ? a[12 + l] : a[9], "rb"))) return 5;
    }
    FILE* fo = fopen(out, "wb");
    if (!fo) return 5;
    int n = 0;
    for (; n < N; ++n) {
        int ok = 1;
        for (int l = 0; l < L; ++l) ok &= fread(buf[l], 1, fs[l], fi[l]) == fs[l];
        if (!ok) break;
        if (sched_apply(changes, n, c)) return 1;
        for (int l = 0; l < L; ++l) {
            hl_frame_video_fill(f, HL_VIDEO_CHROMA_YUV420, W << l, H << l, buf[l], fs[l]);
            f->encoding = sched_type(types, n);
            int e = hl_codec_encode(c, (hl_frame_t*)f, r);
            if (e) {
                fprintf(stderr, "encode err %d (%s) at frame %d\n", e, err_name(e), n);
                return 6;
            }
            if (!svc || l == L - 1) put(c, r, fo);
            else if (r->type & HL_CODEC_RESULT_TYPE_HDR) fwrite(c->hdr_bytes, 1, c->hdr_bytes_count, fo);
        }
    }
    for (;;) { /* the plugin's look-ahead: the frames it still holds */
        int e = hl_codec_264_gfx950_flush(c, r);
        if (e) {
            fprintf(stderr, "flush err %d (%s)\n", e, err_name(e));
            return 6;
        }
        if (!(r->type & (HL_CODEC_RESULT_TYPE_HDR | HL_CODEC_RESULT_TYPE_DATA))) break;
        put(c, r, fo);
    }
    fclose(fo);
    for (int l = 0; l < L; ++l) {
        fclose(fi[l]);
        free(buf[l]);
    }
    hl_object_unref(r);
    hl_object_unref(c);
    hl_object_unref(f);
    printf("{\"frames\": %d, \"layers\": %d}\n", n, L);
    return 0;
}
