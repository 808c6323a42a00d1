/* symsync_rate_cpu.c -- one-core rate of a plain-C RESTATEMENT of the timing recovery loop (Gardner detector, PI filter, modulo-1
 * counter, polyphase or linear interpolator) for notes/symsync.md. It is not the reference's loop: that one calls VOLK for the dot
 * product, which is not available here; this one uses a scalar float loop the compiler may vectorise.
 * build: cc -O3 -march=native -o symsync_rate_cpu tools/symsync_rate_cpu.c -lm      usage: symsync_rate_cpu [polyphase 0/1] [nsyms] */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#define NS 128
#define L 21
static float bank[NS][L];

static double rrc(double t, double a)
{
    if (t == 0.0) return 1.0 - a + 4.0 * a / M_PI;
    if (fabs(fabs(4.0 * a * t) - 1.0) < 1e-9) return a / sqrt(2.0) * ((1.0 + 2.0 / M_PI) * sin(M_PI / (4.0 * a)) + (1.0 - 2.0 / M_PI) * cos(M_PI / (4.0 * a)));
    return (sin(M_PI * t * (1.0 - a)) + 4.0 * a * t * cos(M_PI * t * (1.0 + a))) / (M_PI * t * (1.0 - 16.0 * a * a * t * t));
}

static inline void interp(const float* in, int m_k, double mu, int poly, float* re, float* im)
{
    if (poly) {
        int idx = (int)floor(NS * mu);
        if (idx < 0) idx = 0;
        if (idx > NS - 1) idx = NS - 1;
        const float* x = in + 2 * (m_k + 2 - L);
        float ar = 0.0f, ai = 0.0f;
        for (int t = 0; t < L; t++) { ar += x[2 * t] * bank[idx][t]; ai += x[2 * t + 1] * bank[idx][t]; }
        *re = ar; *im = ai;
    } else {
        const float m = (float)mu;
        *re = m * in[2 * (m_k + 1)] + (1 - m) * in[2 * m_k];
        *im = m * in[2 * (m_k + 1) + 1] + (1 - m) * in[2 * m_k + 1];
    }
}

int main(int argc, char** argv)
{
    const int poly = argc > 1 ? atoi(argv[1]) : 1, nsyms = argc > 2 ? atoi(argv[2]) : 4000000, sps = 2, H = poly ? L : 2;
    const int n_in = nsyms * sps + H;
    double sum = 0.0;
    static double h[NS * L];
    for (int i = 0; i < 2 * NS * sps * 5 + 1; i++) { h[i] = rrc((double)(i - NS * sps * 5) / (NS * sps), 0.2); sum += h[i]; }
    for (int i = 0; i < NS; i++)
        for (int j = 0; j < L; j++) bank[i][L - 1 - j] = (float)(h[i + j * NS] * NS / sum);
    float* in = calloc((size_t)2 * n_in, sizeof(float));
    float* out = calloc((size_t)2 * nsyms, sizeof(float));
    unsigned s = 1;
    for (int i = 2 * H; i < 2 * n_in; i++) { s = s * 1664525u + 1013904223u; in[i] = ((s >> 9) / 8388608.0f - 0.5f) * 2.0f; }
    const float K1 = -0.025426012f, K2 = -0.000101704034f;
    double best = 1e30;
    int k = 0;
    for (int rep = 0; rep < 5; rep++) {
        double vi = 0.0, cnt = 0.5, mu = 0.0;
        int jump = sps, n = H + 1;
        float lr = in[2 * H], li = in[2 * H + 1];
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        k = 0;
        while (n + jump < n_in && k < nsyms) {
            n += jump;
            const int m_k = n - 1;
            float orr, oi, zr, zi;
            interp(in, m_k, mu, poly, &orr, &oi);
            interp(in, m_k - sps / 2, mu, poly, &zr, &zi);
            out[2 * k] = orr; out[2 * k + 1] = oi;
            const float e = zr * (lr - orr) + zi * (li - oi);
            lr = orr; li = oi; k++;
            const double vp = K1 * e;
            vi += K2 * e;
            const double W1 = 0.5 + vp + vi, W2 = 0.5 + vi;
            if (!(W1 > 0.0 && W2 > 0.0)) break;
            jump = (int)(floor((cnt - W1) / W2) + 2);
            if (jump > 1) { const double cb = cnt - W1 - (jump - 2) * W2; mu = cb / W2; cnt = cb - W2 + 1; }
            else { mu = cnt / W1; cnt = cnt - W1 + 1; }
        }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        const double dt = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
        if (dt < best) best = dt;
    }
    printf("{\"restatement\": true, \"interp\": \"%s\", \"symbols\": %d, \"seconds\": %.6f, \"msym_per_s\": %.3f, \"checksum\": %.6f}\n",
           poly ? "polyphase" : "linear", k, best, k / best * 1e-6, (double)out[2 * (k / 2)]);
    free(in); free(out);
    return 0;
}
