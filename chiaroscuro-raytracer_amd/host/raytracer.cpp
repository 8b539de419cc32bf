// raytracer.cpp -- host side of RayTracer (src/rayTracer.cpp), GPU render loop.
#include "raytracer.hpp"

#include "checkpoint.hpp"
#include "exr.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include <zlib.h>

namespace chiaro {

cr_camera make_camera(vec3 eye, vec3 center, vec3 up, float yview, unsigned xres, unsigned yres) {
    // rayTracer.cpp:41-43
    float z = 1.f;
    float y = z * 0.5f * yview;
    float x = y * ((float)xres / (float)yres);
    // gtc/matrix_transform.inl:521-546 lookAtRH, upper 3x3 as m[col][row]
    const vec3 f = normalize(center - eye);
    const vec3 s = normalize(cross(f, up));
    const vec3 u = cross(s, f);
    const float m[3][3] = {{s.x, u.x, -f.x}, {s.y, u.y, -f.y}, {s.z, u.z, -f.z}};
    // func_matrix.inl:272-294
    const float ood = 1.f / (+m[0][0] * (m[1][1] * m[2][2] - m[2][1] * m[1][2])
                             - m[1][0] * (m[0][1] * m[2][2] - m[2][1] * m[0][2])
                             + m[2][0] * (m[0][1] * m[1][2] - m[1][1] * m[0][2]));
    float r[3][3];
    r[0][0] = +(m[1][1] * m[2][2] - m[2][1] * m[1][2]) * ood;
    r[1][0] = -(m[1][0] * m[2][2] - m[2][0] * m[1][2]) * ood;
    r[2][0] = +(m[1][0] * m[2][1] - m[2][0] * m[1][1]) * ood;
    r[0][1] = -(m[0][1] * m[2][2] - m[2][1] * m[0][2]) * ood;
    r[1][1] = +(m[0][0] * m[2][2] - m[2][0] * m[0][2]) * ood;
    r[2][1] = -(m[0][0] * m[2][1] - m[2][0] * m[0][1]) * ood;
    r[0][2] = +(m[0][1] * m[1][2] - m[1][1] * m[0][2]) * ood;
    r[1][2] = -(m[0][0] * m[1][2] - m[1][0] * m[0][2]) * ood;
    r[2][2] = +(m[0][0] * m[1][1] - m[1][0] * m[0][1]) * ood;
    // rayTracer.cpp:47-49: (scalar * mat3) * vec3 (type_mat3x3.inl:419-433)
    auto mulv = [](const float a[3][3], vec3 v) {
        return vec3(a[0][0] * v.x + a[1][0] * v.y + a[2][0] * v.z, a[0][1] * v.x + a[1][1] * v.y + a[2][1] * v.z,
                    a[0][2] * v.x + a[1][2] * v.y + a[2][2] * v.z);
    };
    const float sy = 1.f / (float)yres, sx = 1.f / (float)xres;
    float a[3][3], b[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            a[i][j] = r[i][j] * sy;
            b[i][j] = r[i][j] * sx;
        }
    const vec3 dy = mulv(a, vec3(0.f, -2.f * y, 0.f));
    const vec3 dx = mulv(b, vec3(2.f * x, 0.f, 0.f));
    const vec3 lu = mulv(r, vec3(-x, y, -z));
    cr_camera c;
    c.eye[0] = eye.x; c.eye[1] = eye.y; c.eye[2] = eye.z;
    c.left_upper[0] = lu.x; c.left_upper[1] = lu.y; c.left_upper[2] = lu.z;
    c.dx[0] = dx.x; c.dx[1] = dx.y; c.dx[2] = dx.z;
    c.dy[0] = dy.x; c.dy[1] = dy.y; c.dy[2] = dy.z;
    return c;
}

RayTracer::RayTracer(Model &_model, Scene &_scene, int device)
    : scene(_scene), pixels((size_t)_scene.yres * _scene.xres * 3, 0.f), data((size_t)_scene.yres * _scene.xres * 3),
      kdtree(_model, _scene) {
    cr_scene_desc d;
    kdtree.describe(scene, d);
    if (scene.gpus > 1) {
        // GPUs device, device + 1, ...; with fewer GPUs than asked for the ranks wrap
        // around (a device then serves several ranks: same image, no speed-up)
        const int ndev = cr_device_count();
        if (ndev > 0 && (int)scene.gpus > ndev)
            std::cerr << "chiaro: gpus " << scene.gpus << " but " << ndev << " GPU(s) visible; ranks share GPUs\n";
        std::vector<int> devs;
        for (unsigned r = 0; r < scene.gpus; r++) devs.push_back(ndev > 0 ? (device + (int)r) % ndev : device);
        group_ = cr_group_create((int)scene.gpus, devs.data());
        if (cr_group_upload_scene(group_, &d) != CR_OK) {
            std::string msg = std::string("chiaro: scene upload failed: ") + cr_group_last_error(group_);
            cr_group_destroy(group_);
            group_ = nullptr;
            throw std::runtime_error(msg);
        }
        ctx_ = cr_group_ctx(group_, 0);
    } else {
        ctx_ = cr_create(device);
        if (cr_upload_scene(ctx_, &d) != CR_OK) {
            std::string msg = std::string("chiaro: scene upload failed: ") + cr_last_error(ctx_);
            cr_destroy(ctx_);
            ctx_ = nullptr;
            throw std::runtime_error(msg);
        }
    }
    kdtree.attach(ctx_);
}

RayTracer::~RayTracer() {
    if (group_) cr_group_destroy(group_); // owns ctx_
    else cr_destroy(ctx_);
}

void RayTracer::rayTrace(vec3 eye, vec3 center, vec3 up, float yview) { rayTraceLayers(1, eye, center, up, yview); }

void RayTracer::rayTraceLayers(unsigned n, vec3 eye, vec3 center, vec3 up, float yview) {
    if (n < 1) return;
    noiseTracked_ = false; // (these layers keep no moments: a later rayTraceUntil starts over)
    showDenoised_ = false;
    mixedLayers_ = false;
    // rayTracer.cpp:24 -- including the reference's `(lastUp == lastUp)`: a
    // change of `up` alone does not reset the accumulation.
    const bool newLayer = (eye == lastEye) && (center == lastCenter) && (lastUp == lastUp) && (yview == lastYview);
    if (newLayer)
        layers_++;
    else {
        layers_ = 1;
        lastEye = eye;
        lastCenter = center;
        lastUp = up;
        lastYview = yview;
    }
    if (!std::getenv("CHIARO_QUIET"))
        std::cerr << "Camera at (" << eye.x << ", " << eye.y << ", " << eye.z << ") facing: (" << center.x << ", "
                  << center.y << ", " << center.z << ")\nRendering image of size " << scene.xres << "x" << scene.yres
                  << " with " << layers_ * scene.samples << " samples on the GPU...\t";
    const auto t0 = std::chrono::high_resolution_clock::now();
    const cr_camera cam = make_camera(eye, center, up, yview, scene.xres, scene.yres);
    cr_render_params p{};
    p.xres = scene.xres;
    p.yres = scene.yres;
    p.spp = scene.samples;
    p.k = scene.k;
    p.background[0] = scene.background.x;
    p.background[1] = scene.background.y;
    p.background[2] = scene.background.z;
    p.seed = scene.seed;
    p.layer = layers_;
    p.rank = 0;
    p.nranks = 1;
    p.tile = 32;
    // A failed render of several layers may leave the device accumulator holding an unknown number of this
    // call's layers (cr_render_layers blends group after group), and so may a failure past the blend: the
    // next rayTrace then starts over at layer 1, whose blend weight (L - 1 = 0) discards whatever the
    // accumulator holds.  A one-layer call that fails with CR_E_INVALID (parameter checks) or CR_E_OOM (buffer
    // growth) stopped before its only blend -- the pass's last kernel -- so the accumulator still holds
    // layers 1 .. layers_ - 1 intact, and a retry continues at the same layer instead of discarding them.
    auto rollback = [&](int rc) {
        if (n == 1 && (rc == CR_E_INVALID || rc == CR_E_OOM)) layers_--;
        else layers_ = 0;
    };
    if (group_) {
        if (const int rc = n == 1 ? cr_group_render(group_, &cam, &p, pixels.data())
                                  : cr_group_render_layers(group_, &cam, &p, n, pixels.data())) {
            rollback(rc);
            throw std::runtime_error(std::string("chiaro: render failed: ") + cr_group_last_error(group_));
        }
        layers_ += n - 1; // layers p.layer .. p.layer + n - 1 are in the frame
        cr_group_get_counters(group_, &counters_);
    } else {
        if (const int rc = n == 1 ? cr_render(ctx_, &cam, &p, pixels.data())
                                  : cr_render_layers(ctx_, &cam, &p, n, pixels.data())) {
            rollback(rc);
            throw std::runtime_error(std::string("chiaro: render failed: ") + cr_last_error(ctx_));
        }
        layers_ += n - 1; // layers p.layer .. p.layer + n - 1 are in the frame
        cr_get_counters(ctx_, &counters_);
    }
    // rayTracer.cpp:51,66-68 (computed after the render instead of racily inside it)
    maxVal = 0.f;
    for (float v : pixels) maxVal = maxVal > v ? maxVal : v;
    const auto t1 = std::chrono::high_resolution_clock::now();
    lastSeconds_ = std::chrono::duration<double>(t1 - t0).count();
    if (!std::getenv("CHIARO_QUIET")) std::cerr << "took " << lastSeconds_ << " seconds.\n";
}

unsigned RayTracer::rayTraceUntil(float threshold, unsigned maxLayers, vec3 eye, vec3 center, vec3 up, float yview,
                                  float floor, unsigned checkEvery, uint64_t maxAbove) {
    if (group_) throw std::runtime_error("chiaro: rayTraceUntil renders on one GPU (gpus 1)");
    if (maxLayers < 1) throw std::runtime_error("chiaro: rayTraceUntil: maxLayers must be >= 1");
    showDenoised_ = false;
    // rayTraceLayers' rule (rayTracer.cpp:24), and the frame's moments must be complete to go on with it
    const bool newLayer = noiseTracked_ && (eye == lastEye) && (center == lastCenter) && (lastUp == lastUp) &&
                          (yview == lastYview);
    if (newLayer && layers_ >= maxLayers) return layers_;
    mixedLayers_ = false;
    const unsigned first = newLayer ? layers_ + 1 : 1;
    if (!newLayer) {
        lastEye = eye;
        lastCenter = center;
        lastUp = up;
        lastYview = yview;
    }
    const auto t0 = std::chrono::high_resolution_clock::now();
    const cr_camera cam = make_camera(eye, center, up, yview, scene.xres, scene.yres);
    cr_render_params p{};
    p.xres = scene.xres;
    p.yres = scene.yres;
    p.spp = scene.samples;
    p.k = scene.k;
    p.background[0] = scene.background.x;
    p.background[1] = scene.background.y;
    p.background[2] = scene.background.z;
    p.seed = scene.seed;
    p.layer = first;
    p.rank = 0;
    p.nranks = 1;
    p.tile = 32;
    const cr_noise_params np{threshold, floor};
    cr_noise_stats st{};
    momentCam_ = cam;
    if (cr_render_until(ctx_, &cam, &p, 1, maxLayers, checkEvery, &np, maxAbove, pixels.data(), &st) != CR_OK) {
        // (the accumulators may hold any number of this call's layers: the next render starts over)
        layers_ = 0;
        noiseTracked_ = false;
        throw std::runtime_error(std::string("chiaro: render failed: ") + cr_last_error(ctx_));
    }
    layers_ = st.layers;
    noiseTracked_ = true;
    noise_ = st;
    noiseParams_ = np;
    cr_get_counters(ctx_, &counters_);
    maxVal = 0.f;
    for (float v : pixels) maxVal = maxVal > v ? maxVal : v;
    lastSeconds_ = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    return layers_;
}

uint64_t RayTracer::rayTraceAdaptive(float threshold, unsigned maxLayers, vec3 eye, vec3 center, vec3 up, float yview,
                                     float floor, unsigned minLayers, unsigned checkEvery) {
    if (group_) throw std::runtime_error("chiaro: rayTraceAdaptive renders on one GPU (gpus 1)");
    const auto t0 = std::chrono::high_resolution_clock::now();
    const cr_camera cam = make_camera(eye, center, up, yview, scene.xres, scene.yres);
    cr_render_params p{};
    p.xres = scene.xres;
    p.yres = scene.yres;
    p.spp = scene.samples;
    p.k = scene.k;
    p.background[0] = scene.background.x;
    p.background[1] = scene.background.y;
    p.background[2] = scene.background.z;
    p.seed = scene.seed;
    p.layer = 1;
    p.rank = 0;
    p.nranks = 1;
    p.tile = 32;
    const cr_noise_params np{threshold, floor};
    const cr_adaptive_params ap{minLayers, maxLayers, checkEvery};
    // the frame is no progressive state, before or after: whatever follows starts at layer 1
    layers_ = 0;
    noiseTracked_ = false;
    showDenoised_ = false;
    momentCam_ = cam;
    lastEye = lastCenter = lastUp = vec3(FLT_MAX);
    lastYview = -1;
    layerMap_.assign((size_t)scene.xres * scene.yres, 0u);
    cr_adaptive_stats st{};
    if (cr_render_adaptive(ctx_, &cam, &p, &ap, &np, pixels.data(), nullptr, layerMap_.data(), &st) != CR_OK) {
        layerMap_.clear();
        throw std::runtime_error(std::string("chiaro: render failed: ") + cr_last_error(ctx_));
    }
    layers_ = st.layers;
    mixedLayers_ = true;
    adaptive_ = st;
    cr_get_counters(ctx_, &counters_);
    maxVal = 0.f;
    for (float v : pixels) maxVal = maxVal > v ? maxVal : v;
    lastSeconds_ = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    return st.pixel_layers;
}

void RayTracer::denoise(unsigned levels, float sigmaL, float sigmaZ, float sigmaA, unsigned normalSquarings) {
    if (group_) throw std::runtime_error("chiaro: denoise filters on one GPU (gpus 1)");
    if (!layers_ || !(noiseTracked_ || mixedLayers_))
        throw std::runtime_error("chiaro: denoise: the frame's moments are not complete (render it with rayTraceUntil "
                                 "or rayTraceAdaptive)");
    const cr_denoise_params dp{levels, sigmaL, sigmaZ, sigmaA, normalSquarings};
    denoised_.resize(pixels.size());
    if (cr_denoise(ctx_, &momentCam_, scene.xres, scene.yres, layers_, scene.samples, &dp,
                   mixedLayers_ ? layerMap_.data() : nullptr, denoised_.data(), nullptr) != CR_OK)
        throw std::runtime_error(std::string("chiaro: denoise failed: ") + cr_last_error(ctx_));
    showDenoised_ = true;
}

uint32_t RayTracer::rayTraceTemporal(vec3 eye, vec3 center, vec3 up, float yview, unsigned layers,
                                     unsigned denoiseLevels) {
    if (group_) throw std::runtime_error("chiaro: rayTraceTemporal renders on one GPU (gpus 1)");
    if (layers < 1) throw std::runtime_error("chiaro: rayTraceTemporal: layers must be >= 1");
    const auto t0 = std::chrono::high_resolution_clock::now();
    const cr_camera cam = make_camera(eye, center, up, yview, scene.xres, scene.yres);
    cr_render_params p{};
    p.xres = scene.xres;
    p.yres = scene.yres;
    p.spp = scene.samples;
    p.k = scene.k;
    p.background[0] = scene.background.x;
    p.background[1] = scene.background.y;
    p.background[2] = scene.background.z;
    p.seed = scene.seed + temporalFrames_;
    p.layer = 1;
    p.rank = 0;
    p.nranks = 1;
    p.tile = 32;
    cr_temporal_params tp;
    cr_temporal_params_default(&tp);
    cr_denoise_params dp;
    cr_denoise_params_default(&dp);
    dp.levels = denoiseLevels;
    // the frame is no progressive state, before or after: whatever follows starts at layer 1
    layers_ = 0;
    noiseTracked_ = false;
    mixedLayers_ = false;
    showDenoised_ = false;
    lastEye = lastCenter = lastUp = vec3(FLT_MAX);
    lastYview = -1;
    denoised_.resize(pixels.size());
    countMap_.assign((size_t)scene.xres * scene.yres, 0u);
    if (cr_render_temporal(ctx_, &cam, &p, layers, &tp, denoiseLevels ? &dp : nullptr, denoised_.data(),
                           countMap_.data()) != CR_OK) {
        countMap_.clear();
        throw std::runtime_error(std::string("chiaro: render failed: ") + cr_last_error(ctx_));
    }
    temporalFrames_++;
    showDenoised_ = true;
    cr_get_counters(ctx_, &counters_);
    maxVal = 0.f;
    for (float v : denoised_) maxVal = maxVal > v ? maxVal : v;
    uint32_t least = 0;
    for (uint32_t k : countMap_)
        if (k && (!least || k < least)) least = k;
    lastSeconds_ = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    return least;
}

// radiance() and gather(): cr_radiance / cr_gather of layers 1 .. layers with the Scene's sampling
static cr_radiance_params radiance_params(const Scene &scene) {
    cr_radiance_params p{};
    p.spp = scene.samples;
    p.k = scene.k;
    p.background[0] = scene.background.x;
    p.background[1] = scene.background.y;
    p.background[2] = scene.background.z;
    p.seed = scene.seed;
    p.layer = 1;
    p.id0 = 0;
    return p;
}
void RayTracer::radiance(const float *orig, const float *dir, uint32_t n, unsigned layers, float *out) {
    if (group_) throw std::runtime_error("chiaro: radiance runs on one GPU (gpus 1)");
    const cr_radiance_params p = radiance_params(scene);
    if (cr_radiance(ctx_, n, orig, dir, &p, layers, out, nullptr) != CR_OK)
        throw std::runtime_error(std::string("chiaro: radiance failed: ") + cr_last_error(ctx_));
    cr_get_counters(ctx_, &counters_);
}
void RayTracer::gather(const float *pos, const float *nrm, uint32_t n, unsigned layers, float *out) {
    if (group_) throw std::runtime_error("chiaro: gather runs on one GPU (gpus 1)");
    const cr_radiance_params p = radiance_params(scene);
    if (cr_gather(ctx_, n, pos, nrm, &p, layers, out, nullptr) != CR_OK)
        throw std::runtime_error(std::string("chiaro: gather failed: ") + cr_last_error(ctx_));
    cr_get_counters(ctx_, &counters_);
}

// bakeProbes() and sampleProbes(): cr_probe_sh of layers 1 .. layers with the Scene's sampling, and the grid lookup
void RayTracer::bakeProbes(const float *pos, uint32_t n, unsigned layers, float *shOut) {
    if (group_) throw std::runtime_error("chiaro: bakeProbes runs on one GPU (gpus 1)");
    const cr_radiance_params p = radiance_params(scene);
    if (cr_probe_sh(ctx_, n, pos, &p, layers, shOut, nullptr) != CR_OK)
        throw std::runtime_error(std::string("chiaro: bakeProbes failed: ") + cr_last_error(ctx_));
    cr_get_counters(ctx_, &counters_);
}
void RayTracer::bakeProbes(const cr_probe_grid &grid, unsigned layers, float *shOut) {
    const uint64_t n = (uint64_t)grid.dims[0] * grid.dims[1] * grid.dims[2];
    if (!n || n > 0xffffffffull) throw std::runtime_error("chiaro: bakeProbes: bad probe grid");
    std::vector<float> pos(3 * (size_t)n);
    if (cr_probe_grid_positions(&grid, pos.data()) != CR_OK) throw std::runtime_error("chiaro: bakeProbes: bad probe grid");
    bakeProbes(pos.data(), (uint32_t)n, layers, shOut);
}
void RayTracer::sampleProbes(const cr_probe_grid &grid, const float *sh, const float *pos, const float *nrm, uint32_t m,
                             float *out) {
    if (group_) throw std::runtime_error("chiaro: sampleProbes runs on one GPU (gpus 1)");
    if (cr_probe_sample(ctx_, &grid, sh, m, pos, nrm, out) != CR_OK)
        throw std::runtime_error(std::string("chiaro: sampleProbes failed: ") + cr_last_error(ctx_));
}

// bakeLightmap(): cr_bake with the Scene's sampling; uv null: the grid atlas at the largest cell that fits
static cr_bake_stats bake_with(cr_ctx *ctx, const Scene &scene, size_t n_tris, uint32_t W, uint32_t H, const float *uv,
                               unsigned layers, const cr_adaptive_params *ap, const cr_noise_params *np, unsigned dilate,
                               float *out, float *dilated, uint32_t *layersOut) {
    cr_bake_params p;
    cr_bake_params_default(&p);
    p.width = W, p.height = H;
    p.spp = scene.samples;
    p.k = scene.k;
    p.background[0] = scene.background.x;
    p.background[1] = scene.background.y;
    p.background[2] = scene.background.z;
    p.seed = scene.seed;
    std::vector<float> atlas;
    if (!uv) {
        uint32_t w1 = 0, h1 = 0;
        if (!n_tris || cr_bake_atlas_grid((uint32_t)n_tris, 1, 0.25f, &w1, &h1, nullptr) != CR_OK || !w1 || !h1)
            throw std::runtime_error("chiaro: bakeLightmap: no triangles for a grid atlas");
        const uint32_t cell = std::min(W / w1, H / h1); // (at cell 1 the atlas is cols x rows texels)
        if (!cell) throw std::runtime_error("chiaro: bakeLightmap: the map is smaller than one texel per triangle");
        atlas.resize(6 * n_tris);
        if (cr_bake_atlas_grid((uint32_t)n_tris, cell, 0.25f, &w1, &h1, atlas.data()) != CR_OK)
            throw std::runtime_error("chiaro: bakeLightmap: grid atlas failed");
        const float sx = (float)w1 / (float)W, sy = (float)h1 / (float)H;
        if (w1 != W || h1 != H)
            for (size_t i = 0; i < atlas.size(); i += 2) atlas[i] *= sx, atlas[i + 1] *= sy;
        uv = atlas.data();
    }
    cr_bake_stats st{};
    if (cr_bake(ctx, &p, uv, layers, ap, np, dilate, out, nullptr, layersOut, nullptr, dilated, &st) != CR_OK)
        throw std::runtime_error(std::string("chiaro: bakeLightmap failed: ") + cr_last_error(ctx));
    return st;
}
cr_bake_stats RayTracer::bakeLightmap(uint32_t W, uint32_t H, const float *uv, unsigned layers, unsigned dilate,
                                      float *out, float *dilated) {
    if (group_) throw std::runtime_error("chiaro: bakeLightmap runs on one GPU (gpus 1)");
    const cr_bake_stats st = bake_with(ctx_, scene, kdtree.triangles.size(), W, H, uv, layers, nullptr, nullptr, dilate,
                                       out, dilated, nullptr);
    cr_get_counters(ctx_, &counters_);
    return st;
}
cr_bake_stats RayTracer::bakeLightmap(uint32_t W, uint32_t H, const float *uv, float threshold, unsigned maxLayers,
                                      float floor, unsigned minLayers, unsigned checkEvery, unsigned dilate, float *out,
                                      float *dilated, uint32_t *layersOut) {
    if (group_) throw std::runtime_error("chiaro: bakeLightmap runs on one GPU (gpus 1)");
    const cr_noise_params np{threshold, floor};
    const cr_adaptive_params ap{minLayers, maxLayers, checkEvery};
    const cr_bake_stats st = bake_with(ctx_, scene, kdtree.triangles.size(), W, H, uv, 0, &ap, &np, dilate, out, dilated,
                                       layersOut);
    cr_get_counters(ctx_, &counters_);
    return st;
}

void RayTracer::resetTemporal() {
    if (group_) return; // (no history with gpus > 1)
    if (cr_temporal_reset(ctx_) != CR_OK)
        throw std::runtime_error(std::string("chiaro: temporal reset failed: ") + cr_last_error(ctx_));
    temporalFrames_ = 0;
}

std::vector<float> RayTracer::noiseMap() {
    if (!noiseTracked_) throw std::runtime_error("chiaro: noiseMap: the frame is not a rayTraceUntil render");
    std::vector<float> err((size_t)scene.xres * scene.yres);
    cr_noise_stats st{};
    if (cr_noise(ctx_, scene.xres, scene.yres, layers_, scene.samples, &noiseParams_, err.data(), &st) != CR_OK)
        throw std::runtime_error(std::string("chiaro: noise map failed: ") + cr_last_error(ctx_));
    return err;
}

uint8_t *RayTracer::getData() { return data.data(); }

void RayTracer::saveCheckpoint(const char *path) const {
    if (!layers_) throw std::runtime_error("checkpoint: nothing rendered yet");
    if (mixedLayers_) throw std::runtime_error("checkpoint: an adaptive frame holds no single layer count to resume from");
    chiaro_checkpoint h{};
    h.xres = scene.xres;
    h.yres = scene.yres;
    h.samples = scene.samples;
    h.k = (uint32_t)scene.k;
    h.seed = scene.seed;
    h.layers = layers_;
    const vec3 *v[3] = {&lastEye, &lastCenter, &lastUp};
    float *dst[3] = {h.eye, h.center, h.up};
    for (int i = 0; i < 3; i++) {
        dst[i][0] = v[i]->x;
        dst[i][1] = v[i]->y;
        dst[i][2] = v[i]->z;
    }
    h.yview = lastYview;
    h.background[0] = scene.background.x;
    h.background[1] = scene.background.y;
    h.background[2] = scene.background.z;
    h.scene = scene_fingerprint(kdtree);
    checkpoint_write(path, h, pixels.data());
}

void RayTracer::resume(const char *path) {
    chiaro_checkpoint h{};
    checkpoint_read(path, h, nullptr);
    if (h.xres != scene.xres || h.yres != scene.yres || h.samples != scene.samples || h.k != (uint32_t)scene.k ||
        h.seed != scene.seed || h.background[0] != scene.background.x || h.background[1] != scene.background.y ||
        h.background[2] != scene.background.z)
        throw std::runtime_error("resume: the checkpoint is of another frame size / spp / depth / seed / background");
    if (h.scene != scene_fingerprint(kdtree)) throw std::runtime_error("resume: the checkpoint is of another scene");
    if (!h.layers) throw std::runtime_error("resume: empty checkpoint");
    checkpoint_read(path, h, pixels.data());
    const int rc = group_ ? cr_group_set_accumulator(group_, scene.xres, scene.yres, pixels.data())
                          : cr_set_accumulator(ctx_, scene.xres, scene.yres, pixels.data());
    if (rc != CR_OK)
        throw std::runtime_error(std::string("resume: ") + (group_ ? cr_group_last_error(group_) : cr_last_error(ctx_)));
    layers_ = h.layers;
    mixedLayers_ = false;
    noiseTracked_ = false; // (the checkpoint holds the frame only)
    showDenoised_ = false;
    lastEye = vec3(h.eye[0], h.eye[1], h.eye[2]);
    lastCenter = vec3(h.center[0], h.center[1], h.center[2]);
    lastUp = vec3(h.up[0], h.up[1], h.up[2]);
    lastYview = h.yview;
    maxVal = 0.f;
    for (float x : pixels) maxVal = maxVal > x ? maxVal : x;
}

// rayTracer.cpp:196-222 (exrdisplay-style): the scalar setup on the host, the
// per-pixel transform on the GPU over the device accumulator of the last layer
// (cr_tonemap; bytes differ from the reference's glibc powf / logf only where a
// value lies within their error of a rounding boundary).
void RayTracer::normalizeImage(float exposure, float defog, float kneeLow, float kneeHigh, float gamma) {
    if (exposure == FLT_MAX) exposure = scene.exposure;
    cr_tonemap_params t;
    cr_tonemap_setup(exposure, defog, kneeLow, kneeHigh, gamma, &t);
    if (showDenoised_) {
        // cr_tonemap reads the device accumulator: it holds the denoised frame for this one call and the rendered
        // frame -- `pixels`, the host copy of exactly those bits -- again afterwards (gpus 1: denoise() saw to that)
        int rc = cr_set_accumulator(ctx_, scene.xres, scene.yres, denoised_.data());
        if (rc == CR_OK) rc = cr_tonemap(ctx_, &t, scene.xres, scene.yres, data.data());
        const int back = cr_set_accumulator(ctx_, scene.xres, scene.yres, pixels.data());
        if (rc != CR_OK || back != CR_OK)
            throw std::runtime_error(std::string("chiaro: tonemap failed: ") + cr_last_error(ctx_));
        return;
    }
    if (group_) {
        if (cr_group_tonemap(group_, &t, scene.xres, scene.yres, data.data()) != CR_OK)
            throw std::runtime_error(std::string("chiaro: tonemap failed: ") + cr_group_last_error(group_));
    } else if (cr_tonemap(ctx_, &t, scene.xres, scene.yres, data.data()) != CR_OK) {
        throw std::runtime_error(std::string("chiaro: tonemap failed: ") + cr_last_error(ctx_));
    }
}

namespace {
bool ends_with(const std::string &s, const char *suf) {
    const size_t n = std::strlen(suf);
    if (s.size() < n) return false;
    for (size_t i = 0; i < n; i++)
        if (std::tolower((unsigned char)s[s.size() - n + i]) != suf[i]) return false;
    return true;
}
void put_be32(std::vector<unsigned char> &v, uint32_t x) {
    for (int i = 3; i >= 0; i--) v.push_back((unsigned char)(x >> (8 * i)));
}
void png_chunk(std::ofstream &o, const char *type, const std::vector<unsigned char> &data) {
    std::vector<unsigned char> buf;
    put_be32(buf, (uint32_t)data.size());
    buf.insert(buf.end(), type, type + 4);
    buf.insert(buf.end(), data.begin(), data.end());
    uLong crc = crc32(0L, Z_NULL, 0);
    crc = crc32(crc, buf.data() + 4, (uInt)(buf.size() - 4));
    put_be32(buf, (uint32_t)crc);
    o.write((const char *)buf.data(), (std::streamsize)buf.size());
}
} // namespace

// rayTracer.cpp:225-279 with this build's own writers (FreeImage is not available):
// float formats keep pixels[0] as the top row, 8-bit formats go through normalizeImage.
void RayTracer::exportImage(const char *filename) {
    const std::string fn(filename);
    const unsigned W = scene.xres, H = scene.yres;
    std::ofstream o(fn, std::ios::binary);
    if (!o) {
        std::cerr << "Couldn't save the image.\nExport failed.\n";
        return;
    }
    if (ends_with(fn, ".pfm")) {
        o << "PF\n" << W << " " << H << "\n-1.0\n";
        for (unsigned y = H; y-- > 0;) o.write((const char *)&shown()[3 * (size_t)y * W], (std::streamsize)(12 * W));
    } else if (ends_with(fn, ".hdr")) { // Radiance RGBE, flat scanlines
        o << "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y " << H << " +X " << W << "\n";
        std::vector<unsigned char> row(4 * (size_t)W);
        for (unsigned y = 0; y < H; y++) {
            for (unsigned x = 0; x < W; x++) {
                const float *p = &shown()[3 * ((size_t)y * W + x)];
                float v = std::max(p[0], std::max(p[1], p[2]));
                unsigned char *e = &row[4 * (size_t)x];
                if (v < 1e-32f) {
                    e[0] = e[1] = e[2] = e[3] = 0;
                } else {
                    int ex;
                    const float sc = std::frexp(v, &ex) * 256.0f / v;
                    e[0] = (unsigned char)(p[0] * sc); e[1] = (unsigned char)(p[1] * sc);
                    e[2] = (unsigned char)(p[2] * sc); e[3] = (unsigned char)(ex + 128);
                }
            }
            o.write((const char *)row.data(), (std::streamsize)row.size());
        }
    } else if (ends_with(fn, ".exr")) { // HALF B, G, R, PIZ: what FreeImage_Save(FIF_EXR, ..., 0) writes
        const std::vector<unsigned char> f = chiaro::exr_encode(shown().data(), (int)W, (int)H);
        o.write((const char *)f.data(), (std::streamsize)f.size());
    } else { // 8-bit: rows of `data` are bottom-up (rayTracer.cpp:217), write top-down
        normalizeImage();
        if (ends_with(fn, ".png")) {
            static const unsigned char sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
            o.write((const char *)sig, 8);
            std::vector<unsigned char> ihdr;
            put_be32(ihdr, W);
            put_be32(ihdr, H);
            ihdr.insert(ihdr.end(), {8, 2, 0, 0, 0});
            png_chunk(o, "IHDR", ihdr);
            std::vector<unsigned char> raw;
            raw.reserve((3 * (size_t)W + 1) * H);
            for (unsigned y = 0; y < H; y++) {
                raw.push_back(0);
                const unsigned char *r = &data[3 * (size_t)(H - 1 - y) * W];
                raw.insert(raw.end(), r, r + 3 * (size_t)W);
            }
            uLongf cl = compressBound((uLong)raw.size());
            std::vector<unsigned char> comp(cl);
            compress2(comp.data(), &cl, raw.data(), (uLong)raw.size(), 6);
            comp.resize(cl);
            png_chunk(o, "IDAT", comp);
            png_chunk(o, "IEND", {});
        } else { // PPM
            o << "P6\n" << W << " " << H << "\n255\n";
            for (unsigned y = 0; y < H; y++) o.write((const char *)&data[3 * (size_t)(H - 1 - y) * W], 3 * (std::streamsize)W);
        }
    }
    if (o) std::cerr << "Render succesfully saved to file " << filename << "\n";
    else std::cerr << "Couldn't save the image.\nExport failed.\n";
}

} // namespace chiaro
