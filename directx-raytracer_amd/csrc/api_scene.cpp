// C ABI, the scene layer (crt_ctx.h maps the units): every crt_scene_* call, and the two that hand a scene to a context through
// the public calls.  No HIP here.
#include "../../include/crt_hip.h"

#include "mem_util.h"
#include "scene.h"

#include <cstdio>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

// (crt_ctx.h's, which this unit leaves out: it would bring the HIP runtime's header)
namespace crtapi {
int fail(crt_ctx* ctx, int code, const char* fmt, ...);
} // namespace crtapi
using crtapi::fail;

struct crt_scene {
    crt::Scene scene;
    // uint32 copies of the int index vectors are not needed: std::vector<int> is reinterpreted like the
    // reference does for its index buffers (R/DXRTRenderer.cpp:314-315)
};

// ------------------------------------------------------------------------------------------- scene layer
int crt_scene_load(const char* path, crt_scene** out, char* err, size_t err_len)
{
    if (!path || !out) return CRT_EINVAL;
    *out = nullptr;
    crt_scene* s = new (std::nothrow) crt_scene();
    if (!s) return CRT_ENOMEM;
    try {
        s->scene.parseSceneFile(path);
    } catch (const std::exception& ex) {
        if (err && err_len) snprintf(err, err_len, "%s", ex.what());
        delete s;
        return std::strstr(ex.what(), "cannot open") ? CRT_EIO : CRT_EPARSE;
    }
    *out = s;
    return CRT_OK;
}

int crt_scene_save(const crt_scene* s, const char* path, char* err, size_t err_len)
{
    if (!s || !path) return CRT_EINVAL;
    try {
        crt::SceneParser::saveBinary(path, s->scene);
    } catch (const std::exception& ex) {
        if (err && err_len) snprintf(err, err_len, "%s", ex.what());
        return CRT_EIO;
    }
    return CRT_OK;
}

int crt_scene_new(crt_scene** out)
{
    if (!out) return CRT_EINVAL;
    *out = new (std::nothrow) crt_scene();
    return *out ? CRT_OK : CRT_ENOMEM;
}

void crt_scene_free(crt_scene* s) { delete s; }

int crt_scene_add_mesh(crt_scene* s, const float* xyz, uint32_t nv, const uint32_t* idx, uint32_t nt, int32_t material_index)
{
    if (!s || (!xyz && nv) || (!idx && nt)) return CRT_EINVAL;
    for (uint32_t i = 0; i < 3 * nt; i++)
        if (idx[i] >= nv) return CRT_EINVAL;
    crt::Mesh& m = s->scene.addObject();
    m.reserve(nv, 3 * static_cast<size_t>(nt));
    for (uint32_t i = 0; i < nv; i++) m.addVertex(crt::Vector(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
    for (uint32_t i = 0; i < 3 * nt; i++) m.addIndex(static_cast<int>(idx[i]));
    m.setMaterialIndex(material_index);
    m.calculateVertexNormals();
    return CRT_OK;
}

int crt_scene_add_light(crt_scene* s, const float pos[3], float intensity)
{
    if (!s || !pos) return CRT_EINVAL;
    s->scene.addLight(crt::Light(crt::Vector(pos[0], pos[1], pos[2]), intensity));
    return CRT_OK;
}

int crt_scene_add_material(crt_scene* s, const crt_material* m)
{
    if (!s || !m) return CRT_EINVAL;
    crt::Material mat;
    mat.setType(static_cast<crt::MaterialType>(m->type <= 4 ? m->type : 0));
    mat.setAlbedo(crt::Vector(m->albedo[0], m->albedo[1], m->albedo[2]));
    mat.setSmoothShading(m->smooth != 0);
    mat.setIor(m->ior);
    s->scene.addMaterial(mat);
    return CRT_OK;
}

uint32_t crt_scene_mesh_count(const crt_scene* s) { return s ? static_cast<uint32_t>(s->scene.getObjects().size()) : 0; }

int crt_scene_mesh(const crt_scene* s, uint32_t i, crt_mesh_view* out)
{
    if (!s || !out || i >= s->scene.getObjects().size()) return CRT_EINVAL;
    const crt::Mesh& m = s->scene.getObjects()[i];
    out->xyz = m.getVertices().empty() ? nullptr : m.getVertices().data()->data();
    out->idx = reinterpret_cast<const uint32_t*>(m.getIndices().data());
    out->normals = m.getVertexNormals().size() == m.getVertices().size() && !m.getVertexNormals().empty()
                       ? m.getVertexNormals().data()->data() : nullptr;
    out->uvs = (m.getUV().size() == m.getVertices().size() && !m.getUV().empty()) ? m.getUV().data()->data() : nullptr;
    out->n_vertices = static_cast<uint32_t>(m.getVertices().size());
    out->n_triangles = static_cast<uint32_t>(m.getIndices().size() / 3);
    out->material_index = m.getMaterialIndex();
    return CRT_OK;
}

uint32_t crt_scene_light_count(const crt_scene* s) { return s ? static_cast<uint32_t>(s->scene.getLights().size()) : 0; }

int crt_scene_light(const crt_scene* s, uint32_t i, crt_light* out)
{
    if (!s || !out || i >= s->scene.getLights().size()) return CRT_EINVAL;
    const crt::Light& l = s->scene.getLights()[i];
    crt::copyBytes(out->pos, l.getPosition().data(), 12);
    out->intensity = l.getIntensity();
    return CRT_OK;
}

uint32_t crt_scene_material_count(const crt_scene* s) { return s ? static_cast<uint32_t>(s->scene.getMaterials().size()) : 0; }

int crt_scene_material(const crt_scene* s, uint32_t i, crt_material* out)
{
    if (!s || !out || i >= s->scene.getMaterials().size()) return CRT_EINVAL;
    const crt::Material& m = s->scene.getMaterials()[i];
    crt::copyBytes(out->albedo, m.getAlbedo().data(), 12);
    out->type = static_cast<uint32_t>(m.getType());
    out->smooth = m.isSmoothShading() ? 1u : 0u;
    out->ior = m.getIor();
    out->texture = m.isTexture() ? s->scene.textureIndexByName(m.getTextureName()) : -1; // getTextureByName, R/CRTScene.cpp:52-63
    return CRT_OK;
}

uint32_t crt_scene_texture_count(const crt_scene* s) { return s ? static_cast<uint32_t>(s->scene.getTextures().size()) : 0; }

int crt_scene_texture_color(const crt_scene* s, uint32_t i, float u, float v, float out_rgb[3])
{
    if (!s || !out_rgb || i >= s->scene.getTextures().size()) return CRT_EINVAL;
    const crt::Vector c = s->scene.getTextures()[i].getColor(u, v);
    crt::copyBytes(out_rgb, c.data(), 12);
    return CRT_OK;
}

int crt_scene_add_texture(crt_scene* s, const char* name, const char* type, const float color_a[3], const float color_b[3], float scalar,
                          const char* file_path)
{
    if (!s || !name || !type) return CRT_EINVAL;
    crt::TextureDesc t;
    t.name = name;
    t.type = type;
    if (t.type != "albedo" && t.type != "edges" && t.type != "checker" && t.type != "bitmap") return CRT_EINVAL;
    if (color_a) t.colorA = crt::Vector(color_a[0], color_a[1], color_a[2]);
    if (color_b) t.colorB = crt::Vector(color_b[0], color_b[1], color_b[2]);
    t.scalar = scalar;
    if (file_path) t.filePath = file_path;
    if (t.typeCode() == 3u) {
        try {
            t.loadBitmap(std::string());
        } catch (const std::exception&) {
            return CRT_EIO;
        }
    }
    s->scene.addTexture(t);
    return CRT_OK;
}

int crt_scene_set_material_texture(crt_scene* s, uint32_t material, const char* texture_name)
{
    if (!s || !texture_name || material >= s->scene.getMaterials().size()) return CRT_EINVAL;
    s->scene.materialsRef()[material].setTextureName(texture_name);
    return CRT_OK;
}

int crt_scene_set_mesh_uvs(crt_scene* s, uint32_t mesh, const float* uvs)
{
    if (!s || !uvs || mesh >= s->scene.getObjects().size()) return CRT_EINVAL;
    crt::Mesh& m = s->scene.objectsRef()[mesh];
    std::vector<crt::Vector> uv(m.getVertices().size());
    for (size_t i = 0; i < uv.size(); i++) uv[i] = crt::Vector(uvs[3 * i], uvs[3 * i + 1], uvs[3 * i + 2]);
    m.setUVs(std::move(uv));
    return CRT_OK;
}

int crt_scene_settings(const crt_scene* s, uint32_t* width, uint32_t* height, float background_rgb[3])
{
    if (!s) return CRT_EINVAL;
    const crt::Settings& st = s->scene.getSettings();
    if (width) *width = static_cast<uint32_t>(st.imageWidth);
    if (height) *height = static_cast<uint32_t>(st.imageHeight);
    if (background_rgb) crt::copyBytes(background_rgb, st.backgroundColor.data(), 12);
    return CRT_OK;
}

int crt_scene_camera_get(const crt_scene* s, float pos[3], float rot[9])
{
    if (!s) return CRT_EINVAL;
    if (pos) crt::copyBytes(pos, s->scene.getCamera().getPosition().data(), 12);
    if (rot) crt::copyBytes(rot, s->scene.getCamera().getRotationMatrix().data(), 36);
    return CRT_OK;
}

int crt_scene_camera_set(crt_scene* s, const float pos[3], const float rot[9])
{
    if (!s) return CRT_EINVAL;
    if (pos) s->scene.getCamera().setPosition(crt::Vector(pos[0], pos[1], pos[2]));
    if (rot) s->scene.getCamera().setRotationMatrix(crt::Matrix(rot[0], rot[1], rot[2], rot[3], rot[4], rot[5], rot[6], rot[7], rot[8]));
    return CRT_OK;
}

#define CAMERA_OP(name, call)                        \
    int name                                         \
    {                                                \
        if (!s) return CRT_EINVAL;                   \
        s->scene.getCamera().call;                   \
        return CRT_OK;                               \
    }
CAMERA_OP(crt_scene_camera_rotate(crt_scene* s, float dyaw, float dpitch), rotate(dyaw, dpitch))
CAMERA_OP(crt_scene_camera_zoom(crt_scene* s, float amount), zoom(amount))
CAMERA_OP(crt_scene_camera_move_forward(crt_scene* s, float d), moveForward(d))
CAMERA_OP(crt_scene_camera_move_right(crt_scene* s, float d), moveRight(d))
CAMERA_OP(crt_scene_camera_pan(crt_scene* s, float deg), pan(deg))
CAMERA_OP(crt_scene_camera_tilt(crt_scene* s, float deg), tilt(deg))
CAMERA_OP(crt_scene_camera_roll(crt_scene* s, float deg), roll(deg))
#undef CAMERA_OP

int crt_scene_camera_pan_around_target(crt_scene* s, float degrees, const float target[3])
{
    if (!s || !target) return CRT_EINVAL;
    s->scene.getCamera().panAroundTarget(degrees, crt::Vector(target[0], target[1], target[2]));
    return CRT_OK;
}

int crt_upload_scene_from(crt_ctx* c, const crt_scene* s)
{
    if (!c) return CRT_EINVAL;
    if (!s) return fail(c, CRT_EINVAL, "scene is NULL");
    const uint32_t nm = crt_scene_mesh_count(s), nl = crt_scene_light_count(s), nmat = crt_scene_material_count(s);
    std::vector<crt_mesh_view> meshes(nm);
    std::vector<crt_light> lights(nl);
    std::vector<crt_material> mats(nmat);
    for (uint32_t i = 0; i < nm; i++) crt_scene_mesh(s, i, &meshes[i]);
    for (uint32_t i = 0; i < nl; i++) crt_scene_light(s, i, &lights[i]);
    for (uint32_t i = 0; i < nmat; i++) crt_scene_material(s, i, &mats[i]);
    int rc = crt_upload_scene(c, meshes.data(), nm, lights.data(), nl, mats.data(), nmat);
    if (rc) return rc;
    std::vector<crt_texture> tex;
    for (const crt::TextureDesc& t : s->scene.getTextures()) {
        crt_texture x{};
        x.type = t.typeCode();
        crt::copyBytes(x.color_a, t.colorA.data(), 12);
        crt::copyBytes(x.color_b, t.colorB.data(), 12);
        x.scalar = t.scalar;
        x.pixels = t.pixels.empty() ? nullptr : t.pixels.data();
        x.width = static_cast<uint32_t>(t.width);
        x.height = static_cast<uint32_t>(t.height);
        x.channels = static_cast<uint32_t>(t.channels);
        tex.push_back(x);
    }
    rc = crt_set_textures(c, tex.data(), static_cast<uint32_t>(tex.size()));
    if (rc) return rc;
    return crt_set_camera_from(c, s);
}

int crt_set_camera_from(crt_ctx* c, const crt_scene* s)
{
    if (!c) return CRT_EINVAL;
    if (!s) return fail(c, CRT_EINVAL, "scene is NULL");
    return crt_set_camera(c, s->scene.getCamera().getPosition().data(), s->scene.getCamera().getRotationMatrix().data());
}
