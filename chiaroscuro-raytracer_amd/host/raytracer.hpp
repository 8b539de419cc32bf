// raytracer.hpp -- RayTracer (mirror of include/rayTracer.hpp:10-41).
//
// Same public API: RayTracer(Model&, Scene&), rayTrace(eye, center, up, yview),
// getData(), maxVal, normalizeImage(...), exportImage(filename).  rayTrace runs
// the render loop on the GPU through libchiaro_hip.so (include/chiaro_hip.h);
// there is no CPU render path in the product.
#pragma once
#include "kdtree.hpp"
#include "scene.hpp"

#include "chiaro_hip.h"

#include <cfloat>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace chiaro {

// Camera basis of src/rayTracer.cpp:41-49 (glm::lookAt + mat3 inverse, glm order).
cr_camera make_camera(vec3 eye, vec3 center, vec3 up, float yview, unsigned xres, unsigned yres);

class RayTracer {
  public:
    // device: HIP device index (scene.gpus > 1: GPUs device .. device + gpus - 1, the
    // layers tile-split over them, cr_group_*).  Throws std::runtime_error when no
    // GPU / the HIP library cannot be used (the product never falls back to the CPU).
    RayTracer(Model &_model, Scene &_scene, int device = 0);
    ~RayTracer();
    RayTracer(const RayTracer &) = delete;
    RayTracer &operator=(const RayTracer &) = delete;

    /* Fill pixels with rays shot on screen centered between eye and center. */
    void rayTrace(vec3 eye, vec3 center, vec3 up = vec3(0.f, 1.f, 0.f), float yview = 1.f);
    /* This build: n calls of rayTrace with the same view, rendered as pass groups
     * (cr_render_layers / cr_group_render_layers with the `gpus` key: several layers per pass group,
     * bit-identical). */
    void rayTraceLayers(unsigned n, vec3 eye, vec3 center, vec3 up = vec3(0.f, 1.f, 0.f), float yview = 1.f);
    /* This build: rayTrace calls with the same view until the frame is quiet enough (cr_render_until): layers
     * are added, the noise checked after each pass group of at most checkEvery layers, until at most maxAbove
     * pixels have a relative error above threshold (include/chiaro_hip.h "noise estimate") or the frame holds
     * maxLayers layers.  The progressive state follows rayTraceLayers' rules: the same view continues the
     * accumulation -- when rayTraceUntil rendered every layer of it, so the moments are complete (a frame that
     * already holds maxLayers is left as it is) -- and anything else starts at layer 1; a later rayTrace /
     * rayTraceLayers continues the frame as usual.  Returns the layer reached; lastNoise() tells whether the
     * target was met.  One GPU only: with gpus > 1 it throws std::runtime_error. */
    unsigned rayTraceUntil(float threshold, unsigned maxLayers, vec3 eye, vec3 center, vec3 up = vec3(0.f, 1.f, 0.f),
                           float yview = 1.f, float floor = 1e-3f, unsigned checkEvery = 4, uint64_t maxAbove = 0);
    /* This build: adaptive sampling (cr_render_adaptive, include/chiaro_hip.h "adaptive sampling"): the view rendered
     * from layer 1, the noise checked every checkEvery layers from minLayers on, and further layers -- at most
     * maxLayers per pixel -- spent only on the pixels whose relative error is still above threshold.  A pixel at or
     * below it is frozen and never re-enters; minLayers guards against freezing on the estimate's low bias at few
     * samples.  Returns the pixel-layers rendered (of xres * yres * maxLayers); layerMap() is each pixel's layer
     * count, lastAdaptive() the statistic.  The frame then holds pixels of different layer counts: it is not a
     * progressive state -- the next rayTrace* call starts at layer 1, and saveCheckpoint refuses it.  One GPU only. */
    uint64_t rayTraceAdaptive(float threshold, unsigned maxLayers, vec3 eye, vec3 center, vec3 up = vec3(0.f, 1.f, 0.f),
                              float yview = 1.f, float floor = 1e-3f, unsigned minLayers = 1, unsigned checkEvery = 1);
    const std::vector<uint32_t> &layerMap() const { return layerMap_; } // [yres][xres]; empty before rayTraceAdaptive
    const cr_adaptive_stats &lastAdaptive() const { return adaptive_; }
    /* This build: the variance-guided a-trous filter (cr_denoise, include/chiaro_hip.h "guide buffers and denoiser")
     * over the frame of the last rayTraceUntil or rayTraceAdaptive -- the renders that keep the frame's moments; an
     * adaptive frame is filtered with its layer map.  Fills the denoised buffer (denoisedData()); exportImage,
     * normalizeImage and getData act on it until the next rayTrace* call.  The rendered frame (pixelData()) and the
     * progressive state are untouched: rayTraceUntil continues bit-identically afterwards.  Throws
     * std::runtime_error when the frame's moments are not complete (any other render), and with gpus > 1. */
    void denoise(unsigned levels = 4, float sigmaL = 4.f, float sigmaZ = .1f, float sigmaA = .1f,
                 unsigned normalSquarings = 5);
    const float *denoisedData() const { return showDenoised_ ? denoised_.data() : nullptr; } // [yres][xres][3]
    /* This build: temporal reprojection (cr_render_temporal, include/chiaro_hip.h "temporal reprojection"): `layers`
     * layers at this view, merged with the history the earlier rayTraceTemporal calls left, carried to this camera
     * through each pixel's first hit.  The seed is scene.seed plus the number of calls since the history began;
     * denoiseLevels > 0 filters the shown frame with that many a-trous levels (the history stays unfiltered).  The
     * result fills the denoised buffer: exportImage, normalizeImage and getData act on it until the next rayTrace*
     * call.  The frame is no progressive state: the next rayTrace / rayTraceLayers / rayTraceUntil starts at layer 1.
     * Returns the smallest non-zero sample count of the frame (countMap()).  One GPU only. */
    uint32_t rayTraceTemporal(vec3 eye, vec3 center, vec3 up = vec3(0.f, 1.f, 0.f), float yview = 1.f,
                              unsigned layers = 1, unsigned denoiseLevels = 0);
    void resetTemporal(); // the next rayTraceTemporal starts a new history (and the seed again at scene.seed)
    const std::vector<uint32_t> &countMap() const { return countMap_; } // [yres][xres]; empty before rayTraceTemporal
    /* This build: radiance queries (cr_radiance / cr_gather, include/chiaro_hip.h "radiance queries"): the light the
     * integrator finds along n caller rays (orig, dir: [n][3], dir not normalised), or the mean incoming radiance under
     * the cosine density at n surface points (pos, nrm: [n][3]; irradiance is pi times it, and offsetting pos off the
     * surface is the caller's job).  Layers 1 .. layers of scene.samples samples each, scene.k, scene.background and
     * scene.seed; ray i draws from the stream of pixel index i.  out [n][3].  The frame, the progressive state and the
     * temporal history are untouched.  One GPU only. */
    void radiance(const float *orig, const float *dir, uint32_t n, unsigned layers, float *out);
    void gather(const float *pos, const float *nrm, uint32_t n, unsigned layers, float *out);
    /* This build: SH irradiance probes (cr_probe_sh / cr_probe_sample, include/chiaro_hip.h "probes").  bakeProbes:
     * the order-2 spherical-harmonic projection of the light arriving at n points (pos [n][3]), or at the probes of
     * a grid in index order, shOut [n][27] = sh[i][k][c]; layers 1 .. layers of scene.samples samples with scene.k,
     * scene.background and scene.seed, probe i on the stream of pixel index i.  sampleProbes: the mean incoming
     * radiance under the cosine density (irradiance / pi, what gather returns) at m points (pos, nrm: [m][3]) from
     * the coefficients of the grid's probes, trilinearly interpolated, with no visibility weighting; out [m][3].  The
     * frame, the progressive state and the temporal history are untouched.  One GPU only. */
    void bakeProbes(const float *pos, uint32_t n, unsigned layers, float *shOut);
    void bakeProbes(const cr_probe_grid &grid, unsigned layers, float *shOut);
    void sampleProbes(const cr_probe_grid &grid, const float *sh, const float *pos, const float *nrm, uint32_t m,
                      float *out);
    /* This build: lightmap baking (cr_bake, include/chiaro_hip.h "lightmap baking").  The W x H lightmap over the
     * lightmap UVs uv ([triangles][6], the scene's triangle order): the mean incoming radiance under the cosine
     * density at the surface point under each covered texel's centre (times pi and the albedo: the caller's), texel
     * y * W + x on the stream of pixel index y * W + x, `layers` layers of scene.samples samples with scene.k,
     * scene.background and scene.seed.  uv null: the grid atlas of the scene's triangles (cr_bake_atlas_grid, gutter
     * 0.25) with the largest cell that fits W x H, in the map's top-left corner.  out [H][W][3]; dilated
     * [H][W][3], when given, is out after `dilate` gutter-filling passes.  The adaptive overload renders further
     * layers only for the texels whose error is above threshold (rayTraceAdaptive's parameters) and returns the
     * (texel, layer) pairs rendered; layersOut [H][W] may be null.  The frame, the progressive state and the temporal
     * history are untouched.  One GPU only, no back faces. */
    cr_bake_stats bakeLightmap(uint32_t W, uint32_t H, const float *uv, unsigned layers, unsigned dilate, float *out,
                               float *dilated = nullptr);
    cr_bake_stats bakeLightmap(uint32_t W, uint32_t H, const float *uv, float threshold, unsigned maxLayers, float floor,
                               unsigned minLayers, unsigned checkEvery, unsigned dilate, float *out,
                               float *dilated = nullptr, uint32_t *layersOut = nullptr);
    /* The statistic of the last rayTraceUntil's last check, and the error map [yres][xres] of its frame. */
    const cr_noise_stats &lastNoise() const { return noise_; }
    std::vector<float> noiseMap();
    /* Get RGB (24 bits per pixel) image location. */
    uint8_t *getData();
    /* The biggest single pixel color generated in last rayTrace() call. */
    float maxVal = 0.f;
    /* Normalize image so png and preview look somehow alike to exr output. */
    void normalizeImage(float exposure = FLT_MAX, float defog = 0.f, float kneeLow = 0.f, float kneeHigh = 5.f,
                        float gamma = 2.2f);
    /* Export: .pfm/.exr/.hdr in float, .ppm/.png 8-bit via normalizeImage. */
    void exportImage(const char *filename);

    // --- additions of this build (not in the reference API) ---
    const float *pixelData() const { return pixels.data(); } // [yres][xres][3], row 0 = top
    unsigned layers() const { return layers_; }
    cr_ctx *context() { return ctx_; }          // with gpus > 1: the root GPU's ctx
    cr_group *group() { return group_; }        // gpus > 1, else null
    KDTree &tree() { return kdtree; }
    const cr_counters &lastCounters() const { return counters_; }
    // checkpoint / resume of the progressive state (host/checkpoint.hpp); resume throws
    // std::runtime_error for a checkpoint of another frame, sampling or scene
    void saveCheckpoint(const char *path) const;
    void resume(const char *path);
    double lastSeconds() const { return lastSeconds_; }

  private:
    Scene &scene;
    std::vector<float> pixels; // replaces std::vector<std::vector<glm::vec3>>
    std::vector<uint8_t> data;
    KDTree kdtree;
    cr_ctx *ctx_ = nullptr;
    cr_group *group_ = nullptr;
    cr_counters counters_{};
    cr_noise_stats noise_{};
    cr_noise_params noiseParams_{0.f, 0.f}; // of the last rayTraceUntil (floor 0: none yet)
    bool noiseTracked_ = false;             // every layer of the frame came from rayTraceUntil (moments complete)
    cr_adaptive_stats adaptive_{};
    std::vector<uint32_t> layerMap_;
    bool mixedLayers_ = false; // the frame is rayTraceAdaptive's: its pixels hold different layer counts
    cr_camera momentCam_{};    // the camera of the last rayTraceUntil / rayTraceAdaptive (denoise's guides)
    std::vector<float> denoised_;
    bool showDenoised_ = false; // denoise() / rayTraceTemporal() ran on this frame: export / normalize / getData act on denoised_
    std::vector<uint32_t> countMap_;
    uint32_t temporalFrames_ = 0; // rayTraceTemporal calls since the history began: the next call's seed offset
    const std::vector<float> &shown() const { return showDenoised_ ? denoised_ : pixels; }
    double lastSeconds_ = 0.0;
    // rayTracer.cpp:18-22 progressive-layer state (per instance here, not function-static)
    unsigned layers_ = 0;
    vec3 lastEye{FLT_MAX}, lastCenter{FLT_MAX}, lastUp{FLT_MAX};
    float lastYview = -1;
};

} // namespace chiaro
