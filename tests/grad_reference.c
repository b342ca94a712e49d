/* A plain C restatement of the gradient contract (include/crt_hip.h, "gradients"), for tests/test_gradients.py.  Compile with -O2
 * -ffp-contract=off -fno-fast-math: fused multiply-adds exist only where FMA is written, / and SQRT are correctly rounded.  Built
 * twice: as it stands in float32, the arithmetic the kernels promise bit for bit, and with -DGRAD_DOUBLE in float64, the same
 * formulas with 29 more bits, which the tests hold against torch.autograd and use to measure the float32 build's own error.
 *
 * Both functions take the scene as explicit arrays -- per mesh the first triangle and the first vertex (n_meshes + 1 entries of
 * tri_start: the last one is the triangle total), the world vertices by vertex, the mesh-local indices -- and per record write the
 * record's gradient, its nine vertex contributions {to a | to b | to c} (zeros for an inert record) and whether it is live.  The
 * vertex sums are the caller's business: the kernels add the contributions in float64 in any order. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef GRAD_DOUBLE
typedef double real;
#define REAL_MAX 1.7976931348623157e308
#define FABS fabs
#define SQRT sqrt
#define FMA fma
#else
typedef float real;
#define REAL_MAX 3.402823466e+38f
#define FABS fabsf
#define SQRT sqrtf
#define FMA fmaf
#endif

static int finite1(real x) { return FABS(x) <= REAL_MAX; } /* false for NaN */

static void cross(const real* x, const real* y, real* out)
{
    out[0] = x[1] * y[2] - x[2] * y[1];
    out[1] = x[2] * y[0] - x[0] * y[2];
    out[2] = x[0] * y[1] - x[1] * y[0];
}

/* the triangle's vertices; 0: the ids name no triangle */
static int triangle_of(uint32_t n_meshes, const uint32_t* tri_start, const uint32_t* vert_start, const real* world, const uint32_t* idx,
                       uint32_t inst, uint32_t prim, const real* v[3])
{
    if (inst == 0xFFFFFFFFu || inst >= n_meshes || prim >= tri_start[inst + 1] - tri_start[inst]) return 0;
    const uint32_t* tri = idx + 3 * ((size_t)tri_start[inst] + prim);
    for (int k = 0; k < 3; k++) v[k] = world + 3 * ((size_t)vert_start[inst] + tri[k]);
    return 1;
}

static void contributions(real u, real v, const real* s, real* contrib)
{
    const real w = ((real)1 - u) - v;
    for (int k = 0; k < 3; k++) {
        contrib[k] = -(w * s[k]);
        contrib[3 + k] = -(u * s[k]);
        contrib[6 + k] = -(v * s[k]);
    }
}

/* grad_t / grad_uv may be NULL (zeros).  grad_rays: 8 per record {dL/do, 0, dL/dd, 0}; contrib: 9 per record; live: 1 per record */
void ray_grad_reference(uint32_t n, uint32_t n_meshes, const uint32_t* tri_start, const uint32_t* vert_start, const real* world, const uint32_t* idx,
                        const real* rays, const uint32_t* inst, const uint32_t* prim, const real* t, const real* uv, const real* grad_t,
                        const real* grad_uv, real* grad_rays, real* contrib, uint8_t* live)
{
    for (size_t i = 0; i < n; i++) {
        const real* vtx[3];
        real* out = grad_rays + 8 * i;
        memset(out, 0, 8 * sizeof(real));
        memset(contrib + 9 * i, 0, 9 * sizeof(real));
        live[i] = 0;
        if (!triangle_of(n_meshes, tri_start, vert_start, world, idx, inst[i], prim[i], vtx)) continue;
        const real u = uv[2 * i], v = uv[2 * i + 1], gt = grad_t ? grad_t[i] : (real)0, gu = grad_uv ? grad_uv[2 * i] : (real)0,
                   gv = grad_uv ? grad_uv[2 * i + 1] : (real)0;
        if (!(finite1(t[i]) && finite1(u) && finite1(v) && finite1(gt) && finite1(gu) && finite1(gv))) continue;
        const real* d = rays + 8 * i + 4;
        real e1[3], e2[3], nn[3], pp[3], qq[3], lam[3], tl[3];
        int ok = 1;
        for (int k = 0; k < 3; k++) {
            e1[k] = vtx[1][k] - vtx[0][k];
            e2[k] = vtx[2][k] - vtx[0][k];
        }
        cross(e1, e2, nn);
        cross(d, e2, pp);
        cross(e1, d, qq);
        const real det = -((d[0] * nn[0] + d[1] * nn[1]) + d[2] * nn[2]);
        for (int k = 0; k < 3; k++) {
            const real num = (gt * nn[k] + gu * pp[k]) + gv * qq[k];
            lam[k] = num / det;
            tl[k] = t[i] * lam[k];
            ok = ok && finite1(lam[k]) && finite1(tl[k]);
        }
        if (!ok) continue;
        live[i] = 1;
        for (int k = 0; k < 3; k++) {
            out[k] = lam[k];
            out[4 + k] = tl[k];
        }
        contributions(u, v, lam, contrib + 9 * i);
    }
}

/* grad_points: 4 per record {dL/dp, 0} */
void point_grad_reference(uint32_t n, uint32_t n_meshes, const uint32_t* tri_start, const uint32_t* vert_start, const real* world,
                          const uint32_t* idx, const real* points, const uint32_t* inst, const uint32_t* prim, const real* uv, const real* grad_dist,
                          real* grad_points, real* contrib, uint8_t* live)
{
    for (size_t i = 0; i < n; i++) {
        const real* vtx[3];
        real* out = grad_points + 4 * i;
        memset(out, 0, 4 * sizeof(real));
        memset(contrib + 9 * i, 0, 9 * sizeof(real));
        live[i] = 0;
        if (!triangle_of(n_meshes, tri_start, vert_start, world, idx, inst[i], prim[i], vtx)) continue;
        const real u = uv[2 * i], v = uv[2 * i + 1], g = grad_dist[i];
        if (!(finite1(u) && finite1(v) && finite1(g))) continue;
        const real* p = points + 4 * i;
        real r[3], s[3];
        for (int k = 0; k < 3; k++) {
            const real a = vtx[0][k], e1 = vtx[1][k] - a, e2 = vtx[2][k] - a;
            r[k] = p[k] - FMA(v, e2, FMA(u, e1, a));
        }
        const real len = SQRT((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
        int ok = len > (real)0 && finite1(len);
        for (int k = 0; k < 3; k++) {
            s[k] = g * (r[k] / len);
            ok = ok && finite1(s[k]);
        }
        if (!ok) continue;
        live[i] = 1;
        for (int k = 0; k < 3; k++) out[k] = s[k];
        contributions(u, v, s, contrib + 9 * i);
    }
}
