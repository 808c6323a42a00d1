/* plsync_rate_cpu.c -- a plain-C RESTATEMENT of the per-symbol loop of frame_sync::step (reference lib/pl_frame_sync.cc:66-243)
 * for tools/plsync_rate.py: delay lines, a 25-tap and a 32-tap complex dot product per symbol while not locked, the three-state
 * machine. It is not the reference (which calls VOLK) and exists only to put a one-core number next to the device's. The frame
 * length is fixed (the CCM / SIS path). Returns the number of headers seen; *locked_out = final state is locked. */
#include <math.h>
#include <stdint.h>
#include <string.h>

static void dot(const float* line, int head, int len, const float* taps_im, float* re, float* im)
{   /* sum line[k] * (j taps_im[k]) as a generic complex multiply-accumulate, newest value first */
    float ar = 0.0f, ai = 0.0f;
    for (int k = 0; k < len; k++) {
        const int p = head - k < 0 ? head - k + len : head - k;
        const float xr = line[2 * p], xi = line[2 * p + 1], tr = 0.0f, ti = taps_im[k];
        ar += xr * tr - xi * ti;
        ai += xr * ti + xi * tr;
    }
    *re = ar; *im = ai;
}

int64_t plsync_rate_cpu(const float* x, int64_t n, const float* sof_taps_rev, const float* plsc_taps_rev, int frame_len, int unlock_thresh,
                        int* locked_out)
{
    float delay[2 * 65], sofb[2 * 25], pe[2 * 32], po[2 * 32];
    int dh = 0, sh = 0, eh = 0, oh = 0, state = 0, unlock = 0;
    uint32_t cnt = 0;
    float lr = 0.0f, li = 0.0f;
    int64_t headers = 0;
    memset(delay, 0, sizeof delay); memset(sofb, 0, sizeof sofb); memset(pe, 0, sizeof pe); memset(po, 0, sizeof po);
    for (int64_t i = 0; i < n; i++) {
        const float xr = x[2 * i], xi = x[2 * i + 1];
        cnt++;
        const int locked = state == 2;
        if (locked && cnt + 90 <= (uint32_t)frame_len) continue;
        const float dr = xr * lr + xi * li, di = xr * li - xi * lr; /* conj(in) * last */
        lr = xr; li = xi;
        dh = (dh + 1) % 65; delay[2 * dh] = dr; delay[2 * dh + 1] = di;
        const int old = (dh + 1) % 65; /* 64 symbols ago */
        sh = (sh + 1) % 25; sofb[2 * sh] = delay[2 * old]; sofb[2 * sh + 1] = delay[2 * old + 1];
        if (cnt & 1) { oh = (oh + 1) % 32; po[2 * oh] = dr; po[2 * oh + 1] = di; }
        else { eh = (eh + 1) % 32; pe[2 * eh] = dr; pe[2 * eh + 1] = di; }
        if (locked && cnt < (uint32_t)frame_len) continue;
        float sr, si, pr, pi;
        dot(sofb, sh, 25, sof_taps_rev, &sr, &si);
        if (cnt & 1) dot(po, oh, 32, plsc_taps_rev, &pr, &pi); else dot(pe, eh, 32, plsc_taps_rev, &pr, &pi);
        const float a = hypotf(sr + pr, si + pi), b = hypotf(sr - pr, si - pi), m = a > b ? a : b;
        const int is_peak = locked ? m > 25.0f : m > 30.0f;
        if (is_peak) {
            if (state == 0) state = 1; else if (state == 1 && cnt == (uint32_t)frame_len) state = 2;
            unlock = 0;
        } else if (locked) {
            if (++unlock == unlock_thresh) { state = 0; unlock = 0; }
        }
        if (is_peak || locked) { cnt = 0; if (state != 0) headers++; }
    }
    *locked_out = state == 2;
    return headers;
}
