/* A plain C float32 restatement of the variance contract (include/crt_hip.h, "variance": crt_temporal_variance), for
 * tests/test_variance.py.  Compile with -O2 -ffp-contract=off -fno-fast-math: fused multiply-adds exist only where fmaf is
 * written, / is correctly rounded.
 *
 * variance_temporal_reference: the twelve steps of crt_temporal_accumulate with 4', 5', 7' and 9' of the motion variant, and V1 to
 * V6.  The ray directions of both cameras are inputs (3 floats per pixel, pixel py * w + px: the direction of the pixel-centre
 * ray), so nothing of the ray generation is restated.  prev_point may be NULL (nothing moved); hist_prev and mom_prev may be NULL
 * together (no history); out may be NULL; albedo may be NULL when demodulate == 0.  count (may be NULL) is a debug return: per
 * pixel the number N of taps the spatial estimate of V6 counted, 0 where it did not run. */
#include <math.h>
#include <stdint.h>
#include <string.h>

static float dot3(const float* a, const float* b) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }

static int finite1(float x) { return fabsf(x) <= 3.402823466e+38f; } /* false for NaN */

void variance_temporal_reference(uint32_t w, uint32_t h, const float* cam_cur, const float* cam_prev, const float* dir_cur, const float* dir_prev,
                                 const float* rgb, const float* normal, const float* albedo, const float* t, const float* prev_point,
                                 const float* hist_prev, float* hist_next, const float* mom_prev, float* mom_next, float* variance, float* out,
                                 float* count, float alpha, float depth_tolerance, float normal_threshold, uint32_t max_history,
                                 uint32_t demodulate, float alpha_moments, uint32_t min_history)
{
    const float fw = (float)w, fh = (float)h;
    const float* o_cur = cam_cur;
    const float* o_prev = cam_prev;
    const float* R = cam_prev + 3;
    const int same = memcmp(cam_cur, cam_prev, 12 * sizeof(float)) == 0;
    const float cap = (float)max_history;
    for (uint32_t py = 0; py < h; py++) {
        for (uint32_t px = 0; px < w; px++) {
            const size_t i = (size_t)py * w + px;
            const float* c_in = rgb + 3 * i;
            const float* n = normal + 3 * i;
            const float tp = t[i];
            float* rec = hist_next + 8 * i;
            float a[3] = { 1.0f, 1.0f, 1.0f }, c[3], c_out[3], len_out = 1.0f, l, l2, m1, m2;
            int k, live = 1;
            /* 1: live */
            for (k = 0; k < 3; k++) live = live && finite1(c_in[k]) && finite1(n[k]);
            live = live && finite1(tp) && (n[0] != 0.0f || n[1] != 0.0f || n[2] != 0.0f) && tp > 0.0f;
            if (demodulate)
                for (k = 0; k < 3; k++) live = live && finite1(albedo[3 * i + k]);
            rec[4] = n[0];
            rec[5] = n[1];
            rec[6] = n[2];
            rec[7] = tp;
            if (!live) { /* 3 */
                memcpy(rec, c_in, 3 * sizeof(float));
                rec[3] = 0.0f;
                if (out) memcpy(out + 3 * i, c_in, 3 * sizeof(float));
                mom_next[2 * i] = 0.0f; /* V2 */
                mom_next[2 * i + 1] = 0.0f;
                continue;
            }
            /* 2 */
            for (k = 0; k < 3; k++) {
                if (demodulate) a[k] = fmaxf(albedo[3 * i + k], 1e-3f);
                c[k] = c_in[k] / a[k];
                c_out[k] = c[k];
            }
            l = fmaf(0.0722f, c[2], fmaf(0.7152f, c[1], 0.2126f * c[0])); /* V1 */
            l2 = l * l;
            m1 = l;
            m2 = l2;
            if (hist_prev) {
                float P[3], Pm[3], fx = (float)px, fy = (float)py;
                int have = 1, moved = 0;
                for (k = 0; k < 3; k++) P[k] = o_cur[k] + dir_cur[3 * i + k] * tp; /* 4 */
                if (prev_point) {                                                   /* 4' */
                    const float* m = prev_point + 3 * i;
                    moved = finite1(m[0]) && finite1(m[1]) && finite1(m[2]);
                }
                for (k = 0; k < 3; k++) Pm[k] = moved ? prev_point[3 * i + k] : P[k];
                if (!same || moved) {                                               /* 5', 6, 7' */
                    float v[3], col[3], pc[3], s;
                    for (k = 0; k < 3; k++) v[k] = Pm[k] - o_prev[k];
                    for (k = 0; k < 3; k++) {
                        col[0] = R[k];
                        col[1] = R[3 + k];
                        col[2] = R[6 + k];
                        pc[k] = dot3(col, v);
                    }
                    s = -pc[2];
                    fx = ((pc[0] / s) / (fw / fh) + 1.0f) * 0.5f * fw - 0.5f;
                    fy = (1.0f - pc[1] / s) * 0.5f * fh - 0.5f;
                    have = s > 0.0f && fx > -1.0f && fx < fw && fy > -1.0f && fy < fh;
                }
                if (have) { /* 8, 9, 10 */
                    const float x0 = floorf(fx), y0 = floorf(fy);
                    const float wx = fx - x0, wy = fy - y0;
                    const float limit = depth_tolerance * tp;
                    float W = 0.0f, sum[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, sm1 = 0.0f, sm2 = 0.0f;
                    for (k = 0; k < 4; k++) {
                        const long qx = (long)x0 + (k & 1), qy = (long)y0 + (k >> 1);
                        const float b = ((k & 1) ? wx : 1.0f - wx) * ((k >> 1) ? wy : 1.0f - wy);
                        const float* q;
                        const float* mq;
                        float Pq[3], diff[3];
                        size_t qi;
                        int j, usable = 1;
                        if (qx < 0 || qx >= (long)w || qy < 0 || qy >= (long)h) continue;
                        qi = (size_t)qy * w + (size_t)qx;
                        q = hist_prev + 8 * qi;
                        for (j = 0; j < 8; j++) usable = usable && finite1(q[j]);
                        if (!usable || !(q[3] > 0.0f)) continue;
                        mq = mom_prev + 2 * qi;
                        if (!finite1(mq[0]) || !finite1(mq[1])) continue; /* V3 */
                        for (j = 0; j < 3; j++) {
                            Pq[j] = o_prev[j] + dir_prev[3 * qi + j] * q[7];
                            diff[j] = Pq[j] - Pm[j]; /* 9' */
                        }
                        if (!(fabsf(dot3(n, diff)) <= limit)) continue;
                        if (!(dot3(n, q + 4) >= normal_threshold)) continue;
                        W = W + b;
                        for (j = 0; j < 4; j++) sum[j] = sum[j] + b * q[j];
                        sm1 = sm1 + b * mq[0]; /* V4 */
                        sm2 = sm2 + b * mq[1];
                    }
                    if (W >= 0.01f) { /* 11 */
                        const float L = sum[3] / W;
                        const float at = fmaxf(alpha, 1.0f / (L + 1.0f));
                        for (k = 0; k < 3; k++) {
                            const float hc = sum[k] / W;
                            c_out[k] = fmaf(at, c[k] - hc, hc);
                        }
                        len_out = fminf(L + 1.0f, cap);
                        { /* V5 */
                            const float am = fmaxf(alpha_moments, 1.0f / (L + 1.0f));
                            const float h1 = sm1 / W, h2 = sm2 / W;
                            m1 = fmaf(am, l - h1, h1);
                            m2 = fmaf(am, l2 - h2, h2);
                        }
                    }
                }
            }
            /* 12 */
            for (k = 0; k < 3; k++) {
                rec[k] = c_out[k];
                if (out) out[3 * i + k] = c_out[k] * a[k];
            }
            rec[3] = len_out;
            mom_next[2 * i] = m1;
            mom_next[2 * i + 1] = m2;
        }
    }
    /* V6: the variance, from the records just written */
    for (uint32_t py = 0; py < h; py++) {
        for (uint32_t px = 0; px < w; px++) {
            const size_t i = (size_t)py * w + px;
            const float* rec = hist_next + 8 * i;
            const float* n = rec + 4;
            const float len = rec[3], tp = rec[7];
            const float m1 = mom_next[2 * i], m2 = mom_next[2 * i + 1];
            if (count) count[i] = 0.0f;
            if (!(len > 0.0f)) { /* not live */
                variance[i] = 0.0f;
                continue;
            }
            if (len >= (float)min_history) {
                variance[i] = fmaxf(m2 - m1 * m1, 0.0f);
            } else {
                const float limit = depth_tolerance * tp;
                float P[3], N = 0.0f, A1 = 0.0f, A2 = 0.0f, M1, M2;
                int k, dx, dy;
                for (k = 0; k < 3; k++) P[k] = o_cur[k] + dir_cur[3 * i + k] * tp;
                for (dy = -3; dy <= 3; dy++) {
                    for (dx = -3; dx <= 3; dx++) {
                        const long qx = (long)px + dx, qy = (long)py + dy;
                        size_t qi;
                        if (qx < 0 || qx >= (long)w || qy < 0 || qy >= (long)h) continue;
                        qi = (size_t)qy * w + (size_t)qx;
                        if (dx != 0 || dy != 0) {
                            const float* q = hist_next + 8 * qi;
                            float Pq[3], diff[3];
                            int j, usable = finite1(mom_next[2 * qi]) && finite1(mom_next[2 * qi + 1]);
                            for (j = 0; j < 8; j++) usable = usable && finite1(q[j]);
                            if (!usable || !(q[3] > 0.0f)) continue;
                            for (j = 0; j < 3; j++) {
                                Pq[j] = o_cur[j] + dir_cur[3 * qi + j] * q[7];
                                diff[j] = Pq[j] - P[j];
                            }
                            if (!(fabsf(dot3(n, diff)) <= limit)) continue;
                            if (!(dot3(n, q + 4) >= normal_threshold)) continue;
                        }
                        N = N + 1.0f;
                        A1 = A1 + mom_next[2 * qi];
                        A2 = A2 + mom_next[2 * qi + 1];
                    }
                }
                M1 = A1 / N;
                M2 = A2 / N;
                variance[i] = fmaxf(M2 - M1 * M1, 0.0f) * ((float)min_history / len);
                if (count) count[i] = N;
            }
        }
    }
}
