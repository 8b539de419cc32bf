// ref_hot.cpp -- TEST INFRASTRUCTURE ONLY (oracle/_ref).
//
// Drives the reference's own, unmodified objects of src/kdtree.cpp, src/brdf.cpp,
// src/scene.cpp and src/rayTracer.cpp (linked beside src/mesh.cpp, which supplies
// Mesh's constructor and Texture::getColorAt) to produce the goldens G1-G4 of
// tests/golden/make_ref_golden.py: the kd build, both traversals, Diffuse's
// sampling, Scene::randomLight, and RayTracer::sendRay.
//
// What is NOT the reference's here, and why:
//   * oracle/ref/standin/{assimp/scene.h, FreeImage.h, prng.hpp}: declarations
//     only, of libraries and of a header this image lacks.  The FreeImage bodies
//     below do nothing (exportImage is never called).
//   * Model::Model(Scene &) is empty: the reference's loader needs assimp.  The
//     harness fills model.meshes with one three-vertex Mesh per triangle, built
//     by the reference's own Mesh constructor.
//   * PRNG: a scripted URBG (see prng.hpp).  uniformFloat calls libstdc++'s own
//     std::uniform_real_distribution<float>, as randomLight calls its
//     std::uniform_int_distribution.
//   * hot_send_ray restates ONE line of RayTracer::rayTrace (src/rayTracer.cpp:60-62,
//     the camera sample with its two jitter draws).  hot_raytrace calls the real
//     rayTrace, and the generator checks the two against each other.
//
// This TU alone is compiled with -fno-access-control: it reads KDTree::nodes and
// calls the private RayTracer::sendRay and Scene::Scene(std::string).
#include "model.hpp"
#include "prng.hpp"
#include "rayTracer.hpp"
#include "scene.hpp"

#include <FreeImage.h>
#include <glad/glad.h>
#include <omp.h>

#include <cstdint>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

// ------------------------------------------------------------------ PRNG --
namespace PRNG {
Script script = {nullptr, 0, 0, false};
ScriptedURBG rng[1];
ScriptedURBG::result_type ScriptedURBG::operator()() {
    if (script.used >= script.count) {
        script.overrun = true;
        script.used++;
        return 0u;
    }
    return script.words[script.used++];
}
void setSeed() {}
float uniformFloat(float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng[omp_get_thread_num()]); }
} // namespace PRNG

static void script_set(const uint32_t *words, size_t n) {
    PRNG::script.words = words;
    PRNG::script.count = n;
    PRNG::script.used = 0;
    PRNG::script.overrun = false;
}

// ------------------------------------------------- FreeImage: no-op bodies --
extern "C" {
void FreeImage_Initialise(BOOL) {}
void FreeImage_DeInitialise(void) {}
FREE_IMAGE_FORMAT FreeImage_GetFIFFromFilename(const char *) { return FIF_UNKNOWN; }
FIBITMAP *FreeImage_Allocate(int, int, int, unsigned, unsigned, unsigned) { return nullptr; }
FIBITMAP *FreeImage_AllocateT(FREE_IMAGE_TYPE, int, int, int, unsigned, unsigned, unsigned) { return nullptr; }
unsigned FreeImage_GetPitch(FIBITMAP *) { return 0; }
BYTE *FreeImage_GetBits(FIBITMAP *) { return nullptr; }
BOOL FreeImage_SetPixelColor(FIBITMAP *, unsigned, unsigned, RGBQUAD *) { return 0; }
BOOL FreeImage_Save(FREE_IMAGE_FORMAT, FIBITMAP *, const char *, int) { return 0; }
}

// ------------------------------------------------------------------ Model --
Model::Model(Scene &) {}

// Mesh::setupMesh (src/mesh.cpp:110-134) calls these through glad's pointers,
// which are null without a GL context.
static void no_gl() {
    glad_glGenVertexArrays = [](GLsizei, GLuint *) {};
    glad_glGenBuffers = [](GLsizei, GLuint *) {};
    glad_glBindVertexArray = [](GLuint) {};
    glad_glBindBuffer = [](GLenum, GLuint) {};
    glad_glBufferData = [](GLenum, GLsizeiptr, const void *, GLenum) {};
    glad_glEnableVertexAttribArray = [](GLuint) {};
    glad_glVertexAttribPointer = [](GLuint, GLint, GLenum, GLboolean, GLsizei, const void *) {};
}

struct HotScene {
    Scene *scene = nullptr;
    Model *model = nullptr;
    RayTracer *rt = nullptr;
    std::vector<std::vector<unsigned char>> images; // padded texel copies (getColorAt reads one texel past)
    ~HotScene() {
        delete rt;
        delete model;
        delete scene;
    }
};

// the reference prints its scene summary to std::cout / std::cerr: keep the generator's output clean
struct Quiet {
    std::ostringstream sink;
    std::streambuf *out, *err;
    Quiet() : out(std::cout.rdbuf(sink.rdbuf())), err(std::cerr.rdbuf(sink.rdbuf())) {}
    ~Quiet() {
        std::cout.rdbuf(out);
        std::cerr.rdbuf(err);
    }
};

static glm::vec3 v3(const float *p) { return glm::vec3(p[0], p[1], p[2]); }

extern "C" {

// Scene through the reference's public constructor from `rtc`; one Mesh per triangle in the order given
// (the arrays of OracleScene); bg, when not null, sets Scene::background (no .rtc token sets it).
void *hot_scene_create(const char *rtc, uint32_t ntri, const float *pos, const float *vnrm, const float *uv,
                       const float *kd, const float *ke, const int32_t *tex, int ntex, const int *tw, const int *th,
                       const int *tnc, const unsigned char *const *tdata, const float *bg) {
    Quiet q;
    omp_set_num_threads(1);
    no_gl();
    HotScene *h = new HotScene;
    std::string path(rtc);
    char arg0[] = "ref_hot";
    char *argv[2] = {arg0, &path[0]};
    h->scene = new Scene(2, argv);
    if (bg) h->scene->background = v3(bg);
    for (int i = 0; i < ntex; i++) {
        const size_t bytes = (size_t)tw[i] * th[i] * tnc[i], pad = (size_t)(tw[i] + 1) * tnc[i] + 4;
        std::vector<unsigned char> img(bytes + pad, 0);
        memcpy(img.data(), tdata[i], bytes);
        h->images.push_back(std::move(img));
    }
    h->model = new Model(*h->scene);
    h->model->meshes.reserve(ntri);
    for (uint32_t t = 0; t < ntri; t++) {
        std::vector<Vertex> vs(3);
        for (int c = 0; c < 3; c++) {
            vs[c].Position = v3(pos + 9 * (size_t)t + 3 * c);
            vs[c].Normal = v3(vnrm + 9 * (size_t)t + 3 * c);
            vs[c].TexCoords = glm::vec2(uv[6 * (size_t)t + 2 * c], uv[6 * (size_t)t + 2 * c + 1]);
        }
        std::vector<Texture> texs;
        if (tex[t] >= 0) {
            Texture x;
            x.id = 0;
            x.type = "texture_diffuse";
            x.image = h->images[tex[t]].data();
            x.width = tw[tex[t]];
            x.height = th[tex[t]];
            x.nrComponents = tnc[tex[t]];
            texs.push_back(x);
        }
        Color col(glm::vec3(0.f), v3(kd + 3 * (size_t)t), glm::vec3(0.f), v3(ke + 3 * (size_t)t), 1.f);
        h->model->meshes.push_back(Mesh(vs, {0u, 1u, 2u}, texs, col));
    }
    // setupMesh pointed textureDiffuse into the temporary's vector; point it into the stored mesh's own
    for (auto &m : h->model->meshes) m.textureDiffuse = m.textures.empty() ? nullptr : &m.textures[0];
    h->rt = new RayTracer(*h->model, *h->scene);
    return h;
}

void hot_scene_destroy(void *p) { delete (HotScene *)p; }

// what the reference's parser read: k, xres, yres, leaf size, samples; background
void hot_scene_info(void *p, int out[5], float bg[3]) {
    Scene &s = *((HotScene *)p)->scene;
    out[0] = s.k; out[1] = (int)s.xres; out[2] = (int)s.yres; out[3] = (int)s.kdtreeLeafSize; out[4] = (int)s.samples;
    bg[0] = s.background.x; bg[1] = s.background.y; bg[2] = s.background.z;
}

// ---- G1: the tree in pre-order (node, its first child's subtree, its second child's subtree)
static void walk(KDTree &kd, id_t ni, std::vector<uint32_t> &leaf, std::vector<uint32_t> &axis,
                 std::vector<float> &split, std::vector<uint32_t> &count, std::vector<uint32_t> &refs) {
    // (by value: nodes is not resized here, but a copy of four scalars keeps this independent of it)
    const bool is_leaf = kd.nodes[ni].isLeaf;
    leaf.push_back(is_leaf ? 1u : 0u);
    if (is_leaf) {
        axis.push_back(3u);
        split.push_back(0.f);
        count.push_back((uint32_t)kd.nodes[ni].trianglesids.size());
        for (auto t : kd.nodes[ni].trianglesids) refs.push_back((uint32_t)t);
        return;
    }
    axis.push_back((uint32_t)kd.nodes[ni].split.axis);
    split.push_back(kd.nodes[ni].split.position);
    count.push_back(0u);
    const id_t child = kd.nodes[ni].child;
    walk(kd, child, leaf, axis, split, count, refs);
    walk(kd, child + 1, leaf, axis, split, count, refs);
}

// call with null arrays for the sizes, then with arrays of those sizes
void hot_kd_dump(void *p, uint32_t *nnodes, uint32_t *nrefs, uint32_t *is_leaf, uint32_t *axis, float *split,
                 uint32_t *count, uint32_t *refs, float box[6]) {
    KDTree &kd = ((HotScene *)p)->rt->kdtree;
    std::vector<uint32_t> l, a, c, r;
    std::vector<float> s;
    walk(kd, 0, l, a, s, c, r);
    *nnodes = (uint32_t)l.size();
    *nrefs = (uint32_t)r.size();
    if (!is_leaf) return;
    memcpy(is_leaf, l.data(), 4 * l.size());
    memcpy(axis, a.data(), 4 * a.size());
    memcpy(split, s.data(), 4 * s.size());
    memcpy(count, c.data(), 4 * c.size());
    memcpy(refs, r.data(), 4 * r.size());
    for (int i = 0; i < 3; i++) { box[i] = kd.minCoords[i]; box[3 + i] = kd.maxCoords[i]; }
}

uint32_t hot_num_lights(void *p) { return (uint32_t)((HotScene *)p)->scene->lightTriangles.size(); }
void hot_lights(void *p, uint32_t *ids, float *surface) {
    auto &l = ((HotScene *)p)->scene->lightTriangles;
    for (size_t i = 0; i < l.size(); i++) { ids[i] = (uint32_t)l[i].id; surface[i] = l[i].surface; }
}

// ---- G2
void hot_intersect(void *p, uint32_t n, const float *orig, const float *dir, uint32_t *hit, uint32_t *tri,
                   float *bary, float *dist) {
    KDTree &kd = ((HotScene *)p)->rt->kdtree;
    for (uint32_t i = 0; i < n; i++) {
        id_t t = 0;
        glm::vec2 b(0.f);
        float d = 0.f;
        hit[i] = kd.intersectRay(v3(orig + 3 * (size_t)i), v3(dir + 3 * (size_t)i), t, b, d) ? 1u : 0u;
        if (hit[i]) { tri[i] = (uint32_t)t; bary[2 * i] = b.x; bary[2 * i + 1] = b.y; dist[i] = d; }
    }
}
void hot_intersect_shadow(void *p, uint32_t n, const float *orig, const float *dir, const float *dist,
                          const uint32_t *light, uint32_t *occluded) {
    KDTree &kd = ((HotScene *)p)->rt->kdtree;
    for (uint32_t i = 0; i < n; i++)
        occluded[i] = kd.intersectShadowRay(v3(orig + 3 * (size_t)i), v3(dir + 3 * (size_t)i), dist[i], light[i]) ? 1u : 0u;
}

// ---- G3
// Diffuse(color).sample_wi(wi, wo, n, pdf) on two scripted words; sxsy = what uniformFloat(-1, 1) makes of each
void hot_sample_wi(const float *n, const float *color, const uint32_t words[2], float wi[3], float *pdf, float f[3],
                   float sxsy[2], uint32_t *consumed) {
    omp_set_num_threads(1);
    for (int i = 0; i < 2; i++) {
        script_set(words + i, 1);
        sxsy[i] = PRNG::uniformFloat(-1.f, 1.f);
    }
    Diffuse d(v3(color));
    glm::vec3 w(0.f), wo(0.f, 0.f, 1.f);
    script_set(words, 2);
    glm::vec3 r = d.sample_wi(w, wo, v3(n), *pdf);
    wi[0] = w.x; wi[1] = w.y; wi[2] = w.z;
    f[0] = r.x; f[1] = r.y; f[2] = r.z;
    *consumed = (uint32_t)PRNG::script.used | (PRNG::script.overrun ? 0x80000000u : 0u);
}

// Scene::randomLight over nlights lights on scripted words: the index chosen and the words consumed
void hot_random_light(uint32_t nlights, const uint32_t *words, uint32_t nwords, uint32_t *index, uint32_t *consumed) {
    omp_set_num_threads(1);
    Scene s{std::string("")}; // (no such file: defaults, no tokens)
    for (uint32_t i = 0; i < nlights; i++) s.lightTriangles.push_back(LightTriangle(i, 0.f));
    script_set(words, nwords);
    const LightTriangle &l = s.randomLight();
    *index = (uint32_t)(&l - &s.lightTriangles[0]);
    *consumed = (uint32_t)PRNG::script.used | (PRNG::script.overrun ? 0x80000000u : 0u);
}

void hot_uniform(float a, float b, const uint32_t *words, uint32_t nwords, float *out, uint32_t *consumed) {
    omp_set_num_threads(1);
    script_set(words, nwords);
    *out = PRNG::uniformFloat(a, b);
    *consumed = (uint32_t)PRNG::script.used | (PRNG::script.overrun ? 0x80000000u : 0u);
}

// ---- G4
// One camera sample of pixel (x, y): the argument expression of src/rayTracer.cpp:60-62 restated (cam = eye,
// leftUpper, dx, dy as ref_camera computes them), then the reference's own sendRay(eye, dir, 1).  dir_out: the
// camera ray that expression made (what a caller of the radiance query passes to trace the same path).
void hot_send_ray(void *p, const float cam[12], unsigned x, unsigned y, const uint32_t *words, uint32_t nwords,
                  float out[3], float dir_out[3], uint32_t *consumed) {
    omp_set_num_threads(1);
    RayTracer &rt = *((HotScene *)p)->rt;
    const glm::vec3 eye = v3(cam), leftUpper = v3(cam + 3), dx = v3(cam + 6), dy = v3(cam + 9);
    script_set(words, nwords);
    const glm::vec3 dir = leftUpper + (x + PRNG::uniformFloat(0.f, 1.f)) * dx + (y + PRNG::uniformFloat(0.f, 1.f)) * dy;
    glm::vec3 r = rt.sendRay(eye, dir, 1);
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
    dir_out[0] = dir.x; dir_out[1] = dir.y; dir_out[2] = dir.z;
    *consumed = (uint32_t)PRNG::script.used | (PRNG::script.overrun ? 0x80000000u : 0u);
}

// The reference's real RayTracer::rayTrace (one more layer when eye / center / yview repeat) on one scripted
// stream for the whole frame; pixels [yres][xres][3] as RayTracer::pixels holds them afterwards.
void hot_raytrace(void *p, const float *eye, const float *center, const float *up, float yview,
                  const uint32_t *words, uint32_t nwords, float *pixels, uint32_t *consumed) {
    Quiet q;
    omp_set_num_threads(1);
    HotScene *h = (HotScene *)p;
    script_set(words, nwords);
    h->rt->rayTrace(v3(eye), v3(center), v3(up), yview);
    for (unsigned y = 0; y < h->scene->yres; y++)
        for (unsigned x = 0; x < h->scene->xres; x++)
            for (int c = 0; c < 3; c++) pixels[3 * ((size_t)y * h->scene->xres + x) + c] = h->rt->pixels[y][x][c];
    *consumed = (uint32_t)PRNG::script.used | (PRNG::script.overrun ? 0x80000000u : 0u);
}
}
