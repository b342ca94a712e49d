/* Reference of the winding-number queries (crt_winding_numbers*, crt_winding_moments_export; include/crt_hip.h): a plain C
 * restatement of the contract's arithmetic -- the arctangent, the per-triangle term, the brute-force sum, the moment table
 * from an exported tree and the walk over it -- in the order the header writes out.  Compiled by tests/test_winding.py with
 * -O2 -ffp-contract=off -fno-fast-math, so fused multiply-adds exist only where fmaf is written; the GPU results are compared
 * with these bit for bit.  ref_atan2's largest absolute error against float64 atan2 over the grid of the test: 2.95e-7. */
#include "crt_hip.h"

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define REF_PI 0x1.921fb6p+1f
#define REF_PI_2 0x1.921fb6p+0f
#define REF_TWO_PI 6.283185307179586
#define REF_CLUSTER_MAX 4096.0f

static float dot3(const float* a, const float* b) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }

/* the contract's expo(m): the frexp exponent of m, 0 when m is zero or not finite (a NaN is never the largest: m is none) */
static int ref_expo(float m)
{
    int e = 0;
    if (m > 0.0f && m < INFINITY) (void)frexpf(m, &e);
    return e;
}

static float max_abs(float m, float x) { const float ax = fabsf(x); return ax > m ? ax : m; }

float ref_atan2(float y, float x)
{
    const float ay = fabsf(y), ax = fabsf(x);
    const int swap = ay > ax;
    const float mx = swap ? ay : ax, mn = swap ? ax : ay;
    const int ok = (y == y) && (x == x) && (mx > 0.0f) && (mx < INFINITY);
    const float t = mn / mx, s = t * t;
    float p = CRT_ATAN_C6;
    p = fmaf(p, s, CRT_ATAN_C5);
    p = fmaf(p, s, CRT_ATAN_C4);
    p = fmaf(p, s, CRT_ATAN_C3);
    p = fmaf(p, s, CRT_ATAN_C2);
    p = fmaf(p, s, CRT_ATAN_C1);
    p = fmaf(p, s, CRT_ATAN_C0);
    float r = fmaf(t, s * p, t);
    if (swap) r = REF_PI_2 - r;
    if (x < 0.0f) r = REF_PI - r;
    if (!ok) r = 0.0f;
    return y < 0.0f ? -r : r;
}

void ref_atan2_array(uint32_t n, const float* y, const float* x, float* out)
{
    for (uint32_t i = 0; i < n; i++) out[i] = ref_atan2(y[i], x[i]);
}

float ref_half_angle(const float* q, const float* v0, const float* e1, const float* e2)
{
    float a[3], b[3], c[3], f1[3], f2[3], mx = 0.0f;
    for (int k = 0; k < 3; k++) {
        a[k] = v0[k] - q[k];
        b[k] = a[k] + e1[k];
        c[k] = a[k] + e2[k];
        mx = max_abs(max_abs(max_abs(mx, a[k]), b[k]), c[k]);
    }
    /* everything below is dimensionless: the triangle as seen from q, brought to unit size by an exact power of two */
    const int E = ref_expo(mx);
    for (int k = 0; k < 3; k++) {
        a[k] = ldexpf(a[k], -E);
        f1[k] = ldexpf(e1[k], -E);
        f2[k] = ldexpf(e2[k], -E);
        b[k] = a[k] + f1[k];
        c[k] = a[k] + f2[k];
    }
    e1 = f1;
    e2 = f2;
    const float n[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
    const float det = dot3(a, n);
    const float la = sqrtf(dot3(a, a)), lb = sqrtf(dot3(b, b)), lc = sqrtf(dot3(c, c));
    const float m = (la * lb) * lc;
    const float den = ((m + dot3(a, b) * lc) + dot3(b, c) * la) + dot3(c, a) * lb;
    return m == 0.0f ? 0.0f : ref_atan2(det, den);
}

static long long to_fixed(float h) { return llrint((double)h * 0x1p36); }
static float from_fixed(long long sum) { return (float)((double)sum * 0x1p-36 / REF_TWO_PI); }
static int has_nan(const float* p) { return p[0] != p[0] || p[1] != p[1] || p[2] != p[2]; }

/* brute force over the records, in any order */
void ref_winding_exact(const crt_bvh_tri* tris, uint32_t n_tris, uint32_t n, const float* pts, float* w)
{
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < (int64_t)n; i++) {
        const float* q = pts + 4 * i;
        long long sum = 0;
        if (!has_nan(q))
            for (uint32_t t = 0; t < n_tris; t++) sum += to_fixed(ref_half_angle(q, tris[t].v0, tris[t].e1, tris[t].e2));
        w[i] = from_fixed(sum);
    }
}

/* ---- the moment table */

typedef struct { double n[3], a, ap[3]; } moment_sum;

static int finite3(const float* v) { return (v[0] - v[0] == 0.0f) && (v[1] - v[1] == 0.0f) && (v[2] - v[2] == 0.0f); }

static moment_sum node_moments(const crt_bvh_node4q* nodes, uint32_t n4, const crt_bvh_tri* tris, uint32_t i, float* moments)
{
    const crt_bvh_node4q* N = &nodes[i];
    const uint32_t qlo[3] = { N->qlo_x, N->qlo_y, N->qlo_z }, qhi[3] = { N->qhi_x, N->qhi_y, N->qhi_z };
    moment_sum total;
    memset(&total, 0, sizeof(total));
    float* out = moments + 32 * (size_t)i;
    for (int k = 0; k < 4; k++) {
        const int32_t ref = N->ref[k];
        moment_sum s;
        memset(&s, 0, sizeof(s));
        float pt[3] = { 0.0f, 0.0f, 0.0f }, r = 0.0f;
        if (ref != CRT_BVH_EMPTY) {
            if (ref >= 0) {
                if ((uint32_t)ref < n4) s = node_moments(nodes, n4, tris, (uint32_t)ref, moments);
            } else {
                const uint32_t leaf = (uint32_t)~ref, first = leaf >> 3, cnt = leaf & 7u;
                for (uint32_t j = 0; j < cnt; j++) {
                    const crt_bvh_tri* T = &tris[first + j];
                    if (!finite3(T->v0) || !finite3(T->e1) || !finite3(T->e2)) continue;
                    const double e1[3] = { T->e1[0], T->e1[1], T->e1[2] }, e2[3] = { T->e2[0], T->e2[1], T->e2[2] };
                    const double nx = 0.5 * (e1[1] * e2[2] - e1[2] * e2[1]), ny = 0.5 * (e1[2] * e2[0] - e1[0] * e2[2]),
                                 nz = 0.5 * (e1[0] * e2[1] - e1[1] * e2[0]);
                    const double area = sqrt((nx * nx + ny * ny) + nz * nz);
                    s.n[0] += nx; s.n[1] += ny; s.n[2] += nz;
                    s.a += area;
                    for (int a = 0; a < 3; a++) s.ap[a] += area * ((double)T->v0[a] + (e1[a] + e2[a]) / 3.0);
                }
            }
            float rr[3];
            for (int a = 0; a < 3; a++) {
                const float lo = fmaf((float)((qlo[a] >> (8 * k)) & 0xFFu), N->s[a], N->lo[a]);
                const float hi = fmaf((float)((qhi[a] >> (8 * k)) & 0xFFu), N->s[a], N->lo[a]);
                pt[a] = s.a > 0.0 ? (float)(s.ap[a] / s.a) : 0.5f * (lo + hi);
                const float d0 = pt[a] - lo, d1 = hi - pt[a];
                const float q0 = d0 * d0, q1 = d1 * d1;
                rr[a] = q0 > q1 ? q0 : q1;
            }
            r = sqrtf((rr[0] + rr[1]) + rr[2]);
        }
        out[4 * k + 0] = pt[0]; out[4 * k + 1] = pt[1]; out[4 * k + 2] = pt[2]; out[4 * k + 3] = r;
        out[16 + 4 * k + 0] = (float)s.n[0]; out[16 + 4 * k + 1] = (float)s.n[1]; out[16 + 4 * k + 2] = (float)s.n[2];
        out[16 + 4 * k + 3] = 0.0f;
        for (int a = 0; a < 3; a++) { total.n[a] += s.n[a]; total.ap[a] += s.ap[a]; }
        total.a += s.a;
    }
    return total;
}

/* nodes: crt_bvh_export4q; tris: crt_bvh_export; moments: n4 x 32 floats (nodes the root does not reach stay zero) */
void ref_moments(const crt_bvh_node4q* nodes, uint32_t n4, const crt_bvh_tri* tris, float* moments)
{
    memset(moments, 0, sizeof(float) * 32 * (size_t)n4);
    if (n4) (void)node_moments(nodes, n4, tris, 0u, moments);
}

/* the walk over exported nodes and moments */
void ref_winding_tree(const crt_bvh_node4q* nodes, uint32_t n4, const crt_bvh_tri* tris, const float* moments, float beta, uint32_t n,
                      const float* pts, float* w)
{
    const int approx = beta > 0.0f;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < (int64_t)n; i++) {
        const float* q = pts + 4 * i;
        long long sum = 0;
        if (!has_nan(q) && n4) {
            size_t cap = 64, sp = 0;
            int32_t* stack = (int32_t*)malloc(sizeof(int32_t) * cap);
            stack[sp++] = 0;
            while (sp) {
                const int32_t cur = stack[--sp];
                if (cur < 0) {
                    const uint32_t leaf = (uint32_t)~cur, first = leaf >> 3, cnt = leaf & 7u;
                    for (uint32_t j = 0; j < cnt; j++) sum += to_fixed(ref_half_angle(q, tris[first + j].v0, tris[first + j].e1, tris[first + j].e2));
                    continue;
                }
                const float* M = moments + 32 * (size_t)cur;
                for (int k = 0; k < 4; k++) {
                    const int32_t ref = nodes[cur].ref[k];
                    if (ref == CRT_BVH_EMPTY) continue;
                    const float d0[3] = { M[4 * k] - q[0], M[4 * k + 1] - q[1], M[4 * k + 2] - q[2] };
                    const int E = ref_expo(max_abs(max_abs(max_abs(0.0f, d0[0]), d0[1]), d0[2]));
                    const float d[3] = { ldexpf(d0[0], -E), ldexpf(d0[1], -E), ldexpf(d0[2], -E) };
                    const float d2 = dot3(d, d), br = beta * ldexpf(M[4 * k + 3], -E);
                    if (approx && d2 > br * br) {
                        float h = ldexpf((0.5f * dot3(M + 16 + 4 * k, d)) / (d2 * sqrtf(d2)), -2 * E);
                        h = h == h ? h : 0.0f;
                        h = h > REF_CLUSTER_MAX ? REF_CLUSTER_MAX : (h < -REF_CLUSTER_MAX ? -REF_CLUSTER_MAX : h);
                        sum += to_fixed(h);
                    } else {
                        if (sp == cap) stack = (int32_t*)realloc(stack, sizeof(int32_t) * (cap *= 2));
                        stack[sp++] = ref;
                    }
                }
            }
            free(stack);
        }
        w[i] = from_fixed(sum);
    }
}
