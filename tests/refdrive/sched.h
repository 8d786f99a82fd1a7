/* sched.h -- TEST INFRASTRUCTURE: the per-frame schedule of the drivers in
 * this directory (ref_sched_harness.c, drop_in_sched_harness.c). */
#ifndef HL_REFDRIVE_SCHED_H
#define HL_REFDRIVE_SCHED_H
#include <hartallo/hl_codec.h>
#include <hartallo/hl_types.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* hl_frame_t.encoding of frame n: its letter of `types`, AUTO beyond the end */
static HL_VIDEO_ENCODING_TYPE_T sched_type(const char* types, int n)
{
    if (!strcmp(types, "-") || n >= (int)strlen(types)) return HL_VIDEO_ENCODING_TYPE_AUTO;
    switch (types[n]) {
    case 'I': return HL_VIDEO_ENCODING_TYPE_INTRA;
    case 'P': return HL_VIDEO_ENCODING_TYPE_INTER;
    case 'R': return HL_VIDEO_ENCODING_TYPE_RAW;
    case 'L': return HL_VIDEO_ENCODING_TYPE_LOSSLESS;
    default: return HL_VIDEO_ENCODING_TYPE_AUTO;
    }
}

/* applies the "frame:key=value" items of `changes` whose frame is n to the
 * codec; non-zero on an item it cannot parse */
static int sched_apply(const char* changes, int n, struct hl_codec_s* c)
{
    const char* p = changes;
    if (!strcmp(changes, "-")) return 0;
    while (*p) {
        int frame = 0, value = 0;
        char key[32];
        if (sscanf(p, "%d:%31[a-z_]=%d", &frame, key, &value) != 3) {
            fprintf(stderr, "bad schedule item at \"%s\"\n", p);
            return 1;
        }
        if (frame == n) {
            if (!strcmp(key, "me_range")) c->me_range = value;
            else if (!strcmp(key, "deblock")) c->deblock_flag = value;
            else if (!strcmp(key, "early_term")) c->me_early_term_flag = value;
            else if (!strcmp(key, "gop")) c->gop_size = value;
            else if (!strcmp(key, "qp")) c->qp = value;
            else {
                fprintf(stderr, "unknown schedule key \"%s\"\n", key);
                return 1;
            }
        }
        p = strchr(p, ';');
        if (!p) break;
        ++p;
    }
    return 0;
}
#endif
