/* Plain C restatement of steps 2 to 5 of the ambient-occlusion contract (include/crt_hip.h "ambient occlusion", shading mode
 * 120), for tests/test_occlusion_mode.py only: the hash and the generator of the mode-200 paths, the sine of the kernels, the
 * cosine-weighted direction about a normal, the biased origin, the radius from the exported root node and the colour.  Every
 * operation is float32 and rounded on its own; a fused multiply-add stands only where fmaf() / fma() is written.  Build with
 * -O2 -ffp-contract=off -fno-fast-math, as the other tests' *_reference.c files. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

static uint32_t pcg_hash(uint32_t v)
{
    const uint32_t state = v * 747796405u + 2891336453u;
    const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}

static float rng_next(uint32_t* st)
{
    *st = pcg_hash(*st);
    return (float)(*st >> 8) * 0x1p-24f;
}

/* sin(x): reduction by 2 pi in double, odd polynomial to r^23, one rounding to float */
static float sin_contract(float x)
{
    const double xd = (double)x;
    const double k = rint(xd * 0x1.45f306dc9c883p-3);
    double r = fma(-k, 0x1.921fb54442d18p+2, xd);
    r = fma(-k, 0x1.1a62633145c07p-52, r);
    const double r2 = r * r;
    double p = -0x1.761b41316381ap-75;
    p = fma(p, r2, 0x1.71b8ef6dcf572p-66);
    p = fma(p, r2, -0x1.2f49b46814157p-57);
    p = fma(p, r2, 0x1.952c77030ad4ap-49);
    p = fma(p, r2, -0x1.ae7f3e733b81fp-41);
    p = fma(p, r2, 0x1.6124613a86d09p-33);
    p = fma(p, r2, -0x1.ae64567f544e4p-26);
    p = fma(p, r2, 0x1.71de3a556c734p-19);
    p = fma(p, r2, -0x1.a01a01a01a01ap-13);
    p = fma(p, r2, 0x1.1111111111111p-7);
    p = fma(p, r2, -0x1.5555555555555p-3);
    p = p * r2;
    return (float)fma(p, r, r);
}

static void normalize3(float* v)
{
    const float dot = fmaf(v[2], v[2], fmaf(v[1], v[1], v[0] * v[0]));
    const float inv = 1.0f / sqrtf(dot);
    v[0] *= inv;
    v[1] *= inv;
    v[2] *= inv;
}

/* the cosine-weighted direction about the unit normal N for the two uniform numbers (u1, u2) */
static void diffuse_bounce(const float* N, float u1, float u2, float* d)
{
    const float rr = sqrtf(u1), phi = 6.28318530717958648f * u2;
    const float lx = rr * sin_contract(phi + 1.57079632679489662f), ly = rr * sin_contract(phi), lz = sqrtf(fmaxf(0.0f, 1.0f - u1));
    const float sg = copysignf(1.0f, N[2]);
    const float a = -1.0f / (sg + N[2]);
    const float b = N[0] * N[1] * a;
    const float T[3] = { 1.0f + sg * N[0] * N[0] * a, sg * b, -sg * N[0] };
    const float B[3] = { b, sg + N[1] * N[1] * a, -N[1] };
    for (int c = 0; c < 3; c++) d[c] = fmaf(lz, N[c], fmaf(ly, B[c], lx * T[c]));
    normalize3(d);
}

/* n directions from n (normal, u1, u2) */
void ao_ref_bounce(uint32_t n, const float* normals, const float* u1, const float* u2, float* dirs)
{
    for (uint32_t i = 0; i < n; i++) diffuse_bounce(normals + 3 * i, u1[i], u2[i], dirs + 3 * i);
}

/* step 2: Po = (o + d t) moved 1e-3 along N, for n records {ox, oy, oz, tmin, dx, dy, dz, tmax} */
void ao_ref_origins(uint32_t n, const float* rays, const float* t, const float* normals, float* po)
{
    for (uint32_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) {
            const float P = rays[8 * i + c] + rays[8 * i + 4 + c] * t[i];
            po[3 * i + c] = fmaf(normals[3 * i + c], 1e-3f, P);
        }
}

/* step 3: the K directions of every record, dirs[(i * K + s) * 3 ..]; ids[i] is the record's id */
void ao_ref_directions(uint32_t n, const uint32_t* ids, uint32_t K, uint32_t seed, const float* normals, float* dirs)
{
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t s = 0; s < K; s++) {
            uint32_t st = pcg_hash(pcg_hash(pcg_hash(ids[i] ^ pcg_hash(s + pcg_hash(seed)))));
            const float u1 = rng_next(&st), u2 = rng_next(&st);
            diffuse_bounce(normals + 3 * i, u1, u2, dirs + 3 * ((size_t)i * K + s));
        }
}

/* the reach R for option "ao_radius" = v > 0 from node 0 of crt_bvh_export (its first twelve floats: lx0 lx1 ly0 ly1 rx0 rx1 ry0
 * ry1 lz0 lz1 rz0 rz1) */
float ao_ref_radius(uint32_t v, const float* node0)
{
    const float dx = fmaxf(node0[1], node0[5]) - fminf(node0[0], node0[4]);
    const float dy = fmaxf(node0[3], node0[7]) - fminf(node0[2], node0[6]);
    const float dz = fmaxf(node0[9], node0[11]) - fminf(node0[8], node0[10]);
    const float D = sqrtf((dx * dx + dy * dy) + dz * dz);
    return ((float)v / 1000.0f) * D;
}

/* steps 4 and 5 for n hit records: visible[i] of K samples escaped */
void ao_ref_colour(uint32_t n, const uint32_t* visible, uint32_t K, int sky, const float* albedo, const float* miss, const float* direct,
                   float* rgb)
{
    for (uint32_t i = 0; i < n; i++) {
        const float v = (float)((double)visible[i] / (double)K);
        for (int c = 0; c < 3; c++) rgb[3 * i + c] = sky ? fmaf(albedo[3 * i + c] * miss[c], v, direct[3 * i + c]) : v;
    }
}
