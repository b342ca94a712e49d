/* Brute-force restatement of the all-hits ray query of include/crt_hip.h (crt_list_hits*) over exported triangle records
 * (crt_bvh_tri, leaf order), in the kernels' exact operation order: no tree, every triangle, then a qsort of each ray's hits
 * by (prescaled t', global id).  Built by tests/test_list_hits.py with -O2 -ffp-contract=off -fno-fast-math (fused
 * multiply-adds only where fmaf is written, as in the kernels) and loaded with ctypes. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "crt_hip.h"

typedef struct { float x, y, z; } f3;
typedef struct { float t, u, v; uint32_t gid, tri; } hit;

static f3 mk(float x, float y, float z) { f3 r = { x, y, z }; return r; }
static f3 sub(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static float dot(f3 a, f3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static f3 cross(f3 a, f3 b) { return mk(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x))); }

/* the ray queries' Moeller-Trumbore test (traversal.hip.h triTest, division form) with tmin < t < tmax */
static int crosses(f3 o, f3 d, float tmin, float tmax, const crt_bvh_tri* T, float* t, float* u, float* v)
{
    const f3 e1 = mk(T->e1[0], T->e1[1], T->e1[2]), e2 = mk(T->e2[0], T->e2[1], T->e2[2]);
    const f3 p = cross(d, e2);
    const float det = dot(e1, p);
    const float inv = 1.0f / det;
    const f3 s = sub(o, mk(T->v0[0], T->v0[1], T->v0[2]));
    *u = dot(s, p) * inv;
    const f3 q = cross(s, e1);
    *v = dot(d, q) * inv;
    *t = dot(e2, q) * inv;
    return (*u >= 0.0f) & (*v >= 0.0f) & (*u + *v <= 1.0f) & (*t > tmin) & (*t < tmax);
}

static int byTThenGid(const void* pa, const void* pb)
{
    const hit* a = (const hit*)pa;
    const hit* b = (const hit*)pb;
    if (a->t < b->t) return -1;
    if (b->t < a->t) return 1;
    return a->gid < b->gid ? -1 : (a->gid > b->gid ? 1 : 0);
}

/* the record prescaled as the query kernels do (traversal.hip.h queryRay); returns e, 0 in *ok for a record that is not traced */
static int setup(const float* r, f3* o, f3* d, float* tmin, float* tmax, int* ok)
{
    const float m = fmaxf(fmaxf(fabsf(r[4]), fabsf(r[5])), fabsf(r[6]));
    int ex = 0;
    if (m <= 3.40282347e38f) frexpf(m, &ex);
    const int e = ex - 1;
    *o = mk(r[0], r[1], r[2]);
    *d = mk(ldexpf(r[4], -e), ldexpf(r[5], -e), ldexpf(r[6], -e));
    *tmin = ldexpf(r[3], e);
    *tmax = ldexpf(r[7], e);
    *ok = r[0] == r[0] && r[1] == r[1] && r[2] == r[2] && r[4] == r[4] && r[5] == r[5] && r[6] == r[6] && *tmin < *tmax;
    return e;
}

/* pass 1 (records == NULL arrays): offsets[0..n]; pass 2: the sorted records of every ray at offsets[i] */
void ref_list_hits(const crt_bvh_tri* tris, uint32_t n_tris, uint32_t n, const float* rays, uint64_t* offsets, int fill, float* t, float* uv,
                   uint32_t* inst, uint32_t* prim)
{
    long i;
    if (!fill) offsets[0] = 0;
#pragma omp parallel for schedule(dynamic, 16)
    for (i = 0; i < (long)n; i++) {
        f3 o, d;
        float tmin, tmax;
        int ok;
        const int e = setup(rays + 8 * i, &o, &d, &tmin, &tmax, &ok);
        uint32_t c = 0;
        if (!fill) {
            if (ok)
                for (uint32_t k = 0; k < n_tris; k++) {
                    float ht, hu, hv;
                    c += (uint32_t)crosses(o, d, tmin, tmax, tris + k, &ht, &hu, &hv);
                }
            offsets[i + 1] = c; /* counts; summed below */
            continue;
        }
        const uint64_t lo = offsets[i], len = offsets[i + 1] - lo;
        if (!len) continue;
        hit* h = (hit*)malloc(sizeof(hit) * len);
        for (uint32_t k = 0; k < n_tris; k++) {
            float ht, hu, hv;
            if (crosses(o, d, tmin, tmax, tris + k, &ht, &hu, &hv)) {
                h[c].t = ht; h[c].u = hu; h[c].v = hv; h[c].gid = tris[k].gid; h[c].tri = k;
                c++;
            }
        }
        qsort(h, len, sizeof(hit), byTThenGid);
        for (uint64_t k = 0; k < len; k++) {
            t[lo + k] = ldexpf(h[k].t, -e);
            uv[2 * (lo + k)] = h[k].u;
            uv[2 * (lo + k) + 1] = h[k].v;
            inst[lo + k] = tris[h[k].tri].inst;
            prim[lo + k] = tris[h[k].tri].prim;
        }
        free(h);
    }
    if (!fill)
        for (i = 0; i < (long)n; i++) offsets[i + 1] += offsets[i];
}
