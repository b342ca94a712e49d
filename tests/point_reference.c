/* Brute-force restatement of the point queries of include/crt_hip.h (crt_closest_points*, crt_count_hits*, crt_occupancy*)
 * over exported triangle records (crt_bvh_tri, leaf order), in the kernels' exact operation order: no tree, every triangle.
 * Built by tests/test_point_queries.py with -O2 -ffp-contract=off -fno-fast-math (fused multiply-adds only where fmaf is
 * written, as in the kernels) and loaded with ctypes. */
#include <math.h>
#include <stdint.h>

#include "crt_hip.h"

typedef struct { float x, y, z; } f3;

static f3 mk(float x, float y, float z) { f3 r = { x, y, z }; return r; }
static f3 sub(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static float dot(f3 a, f3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static f3 cross(f3 a, f3 b) { return mk(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x))); }
static float clamp01(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }

static float dist2At(f3 ap, f3 ab, f3 ac, float u, float v)
{
    const f3 r = mk(fmaf(-v, ac.x, fmaf(-u, ab.x, ap.x)), fmaf(-v, ac.y, fmaf(-u, ab.y, ap.y)), fmaf(-v, ac.z, fmaf(-u, ab.z, ap.z)));
    return dot(r, r);
}

static float nearestEdge(f3 ap, f3 bp, f3 ab, f3 ac, float* u, float* v)
{
    const f3 bc = sub(ac, ab);
    const float eab = dot(ab, ab), eac = dot(ac, ac), ebc = dot(bc, bc);
    const float tab = eab > 0.0f ? clamp01(dot(ap, ab) / eab) : 0.0f;
    const float tac = eac > 0.0f ? clamp01(dot(ap, ac) / eac) : 0.0f;
    const float tbc = ebc > 0.0f ? clamp01(dot(bp, bc) / ebc) : 0.0f;
    float d2 = dist2At(ap, ab, ac, tab, 0.0f);
    *u = tab; *v = 0.0f;
    const float dac = dist2At(ap, ab, ac, 0.0f, tac);
    if (dac < d2) { *u = 0.0f; *v = tac; d2 = dac; }
    const float ubc = 1.0f - tbc;
    const float dbc = dist2At(ap, ab, ac, ubc, tbc);
    if (dbc < d2) { *u = ubc; *v = tbc; d2 = dbc; }
    return d2;
}

/* closest point of the triangle (a, a + ab, a + ac) to a + ap: barycentrics (u of v1, v of v2), squared distance */
static float closestOnTri(f3 ap, f3 ab, f3 ac, float* u, float* v)
{
    const f3 bp = sub(ap, ab), cp = sub(ap, ac);
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d1 <= 0.0f && d2 <= 0.0f) { *u = 0.0f; *v = 0.0f; return dist2At(ap, ab, ac, *u, *v); }
    if (d3 >= 0.0f && d4 <= d3) { *u = 1.0f; *v = 0.0f; return dist2At(ap, ab, ac, *u, *v); }
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f && d1 - d3 > 0.0f) { *u = d1 / (d1 - d3); *v = 0.0f; return dist2At(ap, ab, ac, *u, *v); }
    if (d6 >= 0.0f && d5 <= d6) { *u = 0.0f; *v = 1.0f; return dist2At(ap, ab, ac, *u, *v); }
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f && d2 - d6 > 0.0f) { *u = 0.0f; *v = d2 / (d2 - d6); return dist2At(ap, ab, ac, *u, *v); }
    const float va = d3 * d6 - d5 * d4, e = d4 - d3, f = d5 - d6;
    if (va <= 0.0f && e >= 0.0f && f >= 0.0f && e + f > 0.0f) { *v = e / (e + f); *u = 1.0f - *v; return dist2At(ap, ab, ac, *u, *v); }
    const float s = (va + vb) + vc;
    if (va > 0.0f && vb > 0.0f && vc > 0.0f && s < INFINITY) {
        *u = vb / s;
        *v = vc / s;
        const float d = dist2At(ap, ab, ac, *u, *v);
        if (s > 0x1p-10f * (dot(ab, ab) * dot(ac, ac))) return d;
        float ue, ve;
        const float de = nearestEdge(ap, bp, ab, ac, &ue, &ve);
        if (de < d) { *u = ue; *v = ve; return de; }
        return d;
    }
    return nearestEdge(ap, bp, ab, ac, u, v);
}

/* one triangle: p, a, ab, ac as 3 floats each; out = {u, v, d2, point x, y, z} */
void ref_closest_on_tri(const float* p, const float* a, const float* ab, const float* ac, float* out)
{
    float u, v;
    const f3 A = mk(a[0], a[1], a[2]), E1 = mk(ab[0], ab[1], ab[2]), E2 = mk(ac[0], ac[1], ac[2]);
    out[2] = closestOnTri(sub(mk(p[0], p[1], p[2]), A), E1, E2, &u, &v);
    out[0] = u;
    out[1] = v;
    out[3] = fmaf(v, E2.x, fmaf(u, E1.x, A.x));
    out[4] = fmaf(v, E2.y, fmaf(u, E1.y, A.y));
    out[5] = fmaf(v, E2.z, fmaf(u, E1.z, A.z));
}

/* crt_closest_points over n_tris records; every output required */
void ref_closest_points(const crt_bvh_tri* tris, uint32_t n_tris, uint32_t n, const float* pts, float* dist, float* point, float* uv,
                        uint32_t* inst, uint32_t* prim)
{
    long i;
#pragma omp parallel for schedule(dynamic, 64)
    for (i = 0; i < (long)n; i++) {
        const float* r = pts + 4 * i;
        const f3 p = mk(r[0], r[1], r[2]);
        const float rmax = r[3];
        float best = rmax * rmax, bu = 0.0f, bv = 0.0f;
        uint32_t bgid = 0xFFFFFFFFu, btri = 0;
        if (r[0] == r[0] && r[1] == r[1] && r[2] == r[2] && rmax >= 0.0f) {
            for (uint32_t k = 0; k < n_tris; k++) {
                const crt_bvh_tri* T = tris + k;
                float u, v;
                const float d2 = closestOnTri(sub(p, mk(T->v0[0], T->v0[1], T->v0[2])), mk(T->e1[0], T->e1[1], T->e1[2]),
                                              mk(T->e2[0], T->e2[1], T->e2[2]), &u, &v);
                if (d2 < best || (d2 == best && T->gid < bgid)) { best = d2; bu = u; bv = v; bgid = T->gid; btri = k; }
            }
        }
        if (bgid != 0xFFFFFFFFu) {
            const crt_bvh_tri* T = tris + btri;
            dist[i] = sqrtf(best);
            point[3 * i + 0] = fmaf(bv, T->e2[0], fmaf(bu, T->e1[0], T->v0[0]));
            point[3 * i + 1] = fmaf(bv, T->e2[1], fmaf(bu, T->e1[1], T->v0[1]));
            point[3 * i + 2] = fmaf(bv, T->e2[2], fmaf(bu, T->e1[2], T->v0[2]));
            inst[i] = T->inst;
            prim[i] = T->prim;
        } else {
            dist[i] = rmax;
            point[3 * i + 0] = p.x; point[3 * i + 1] = p.y; point[3 * i + 2] = p.z;
            inst[i] = prim[i] = 0xFFFFFFFFu;
        }
        uv[2 * i] = bu;
        uv[2 * i + 1] = bv;
    }
}

/* the ray queries' Moeller-Trumbore test (traversal.hip.h triTest, division form) with tmin < t < tmax */
static int crosses(f3 o, f3 d, float tmin, float tmax, const crt_bvh_tri* T)
{
    const f3 e1 = mk(T->e1[0], T->e1[1], T->e1[2]), e2 = mk(T->e2[0], T->e2[1], T->e2[2]);
    const f3 p = cross(d, e2);
    const float det = dot(e1, p);
    const float inv = 1.0f / det;
    const f3 s = sub(o, mk(T->v0[0], T->v0[1], T->v0[2]));
    const float u = dot(s, p) * inv;
    const f3 q = cross(s, e1);
    const float v = dot(d, q) * inv;
    const float t = dot(e2, q) * inv;
    return (u >= 0.0f) & (v >= 0.0f) & (u + v <= 1.0f) & (t > tmin) & (t < tmax);
}

static uint32_t countRay(const crt_bvh_tri* tris, uint32_t n_tris, f3 o, f3 d, float tmin, float tmax)
{
    uint32_t c = 0;
    if (!(o.x == o.x && o.y == o.y && o.z == o.z && d.x == d.x && d.y == d.y && d.z == d.z && tmin < tmax)) return 0;
    for (uint32_t k = 0; k < n_tris; k++) c += (uint32_t)crosses(o, d, tmin, tmax, tris + k);
    return c;
}

/* crt_count_hits: ray records of 8 floats, each prescaled as the query kernels do (traversal.hip.h queryRay): the ray
 * (o, tmin 2^e, d 2^-e, tmax 2^e), e the exponent of the largest |d_i| (frexp's minus one; -1 for zero or non-finite) */
void ref_count_hits(const crt_bvh_tri* tris, uint32_t n_tris, uint32_t n, const float* rays, uint32_t* count)
{
    long i;
#pragma omp parallel for schedule(dynamic, 64)
    for (i = 0; i < (long)n; i++) {
        const float* r = rays + 8 * i;
        const float m = fmaxf(fmaxf(fabsf(r[4]), fabsf(r[5])), fabsf(r[6]));
        int ex = 0;
        if (m <= 3.40282347e38f) frexpf(m, &ex);
        const int e = ex - 1;
        count[i] = countRay(tris, n_tris, mk(r[0], r[1], r[2]), mk(ldexpf(r[4], -e), ldexpf(r[5], -e), ldexpf(r[6], -e)),
                            ldexpf(r[3], e), ldexpf(r[7], e));
    }
}

/* crt_occupancy: point records of 4 floats; counts (may be NULL) receives the three hit counts of each point */
void ref_occupancy(const crt_bvh_tri* tris, uint32_t n_tris, uint32_t n, const float* pts, uint8_t* inside, uint32_t* counts)
{
    static const float D[3][3] = { { CRT_OCCUPANCY_DIR0 }, { CRT_OCCUPANCY_DIR1 }, { CRT_OCCUPANCY_DIR2 } };
    long i;
#pragma omp parallel for schedule(dynamic, 64)
    for (i = 0; i < (long)n; i++) {
        const float* r = pts + 4 * i;
        uint32_t odd = 0;
        for (int k = 0; k < 3; k++) {
            const uint32_t c = countRay(tris, n_tris, mk(r[0], r[1], r[2]), mk(D[k][0], D[k][1], D[k][2]), 0.0f, INFINITY);
            if (counts) counts[3 * i + k] = c;
            odd += c & 1u;
        }
        inside[i] = odd >= 2u ? 1u : 0u;
    }
}
