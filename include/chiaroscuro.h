/*
 * chiaroscuro.h -- C entry points of libchiaroscuro.so, the host mirror of the
 * reference's C++ classes (Scene, Model, KDTree, RayTracer), for FFI callers
 * (ctypes in this repo's tests and bench).  C++ callers use the host headers directly.
 *
 *   chiaro_scene_create      Scene::Scene(argc, argv)              src/scene.cpp:13-72
 *   chiaro_model_create      Model::Model(Scene&)                  src/model.cpp:17-36
 *   chiaro_raytracer_create  RayTracer::RayTracer(Model&, Scene&)  src/rayTracer.cpp:13-15
 *                            (builds KDTree, src/kdtree.cpp:34-108, uploads via cr_upload_scene)
 *   chiaro_raytracer_raytrace RayTracer::rayTrace                  src/rayTracer.cpp:17-74
 *   chiaro_raytracer_raytrace_adaptive / _adaptive / _layer_map
 *                            the same accumulation with further layers only where the frame is still noisy (this
 *                            build; cr_render_adaptive)
 *   chiaro_raytracer_denoise / _denoised
 *                            an edge-avoiding filter over such a frame (this build; cr_denoise)
 *   chiaro_raytracer_raytrace_temporal / _reset_temporal / _count_map, chiaro_preview_set_temporal
 *                            a frame's history carried to a moved camera (this build; cr_render_temporal)
 *   chiaro_raytracer_radiance / _gather
 *                            RayTracer::sendRay (src/rayTracer.cpp:76-135) along caller rays (this build; cr_radiance,
 *                            cr_gather)
 *   chiaro_raytracer_probes / _probes_sample
 *                            order-2 SH irradiance probes and their grid lookup (this build; cr_probe_sh,
 *                            cr_probe_sample)
 *   chiaro_raytracer_bake / _bake_adaptive
 *                            a lightmap of the scene in a second UV set (this build; cr_bake)
 *   chiaro_raytracer_raytrace_until / _noise / _noise_map
 *                            rayTrace repeated until a noise target is met (this build; the accumulation of
 *                            src/rayTracer.cpp:18-33,59-64 with a second-moment frame, cr_render_until)
 *   chiaro_raytracer_data / _maxval / _normalize / _export
 *                            getData / maxVal / normalizeImage / exportImage (rayTracer.cpp:171-279)
 *   chiaro_camera            the camera basis of rayTrace          src/rayTracer.cpp:41-49
 *   chiaro_preview_*         OpenGLPreview's render path without a window: camera,
 *                            key R / TAB / = / - / WASDQE, mouse, scroll, the screen
 *                            texture                               src/openglPreview.cpp:12-257,
 *                                                                  src/camera.cpp
 *
 * Errors: functions return NULL / a negative code; chiaro_last_error() (per thread)
 * gives the message.  C++ exceptions never cross this boundary.
 */
#ifndef CHIAROSCURO_H
#define CHIAROSCURO_H

#include "chiaro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct chiaro_scene chiaro_scene;
typedef struct chiaro_model chiaro_model;
typedef struct chiaro_kdtree chiaro_kdtree;
typedef struct chiaro_raytracer chiaro_raytracer;

typedef struct {
    uint32_t xres, yres, samples, preview_height, leaf_size, seed;
    int32_t k;
    int32_t using_preview;
    float VP[3], LA[3], UP[3], background[3];
    float yview, exposure;
    uint32_t n_invalid; /* tokens reported as "Invalid argument" */
    char obj_path[1024];
    char render_path[1024];
    uint32_t gpus;      /* additive "gpus" key: GPUs the RayTracer splits a layer over */
} chiaro_scene_info;

const char *chiaro_last_error(void);

chiaro_scene *chiaro_scene_create(int argc, const char *const *argv);
int chiaro_scene_info_get(const chiaro_scene *s, chiaro_scene_info *out);
void chiaro_scene_destroy(chiaro_scene *s);

chiaro_model *chiaro_model_create(chiaro_scene *s);
chiaro_model *chiaro_model_load(const char *obj_path);
uint32_t chiaro_model_num_meshes(const chiaro_model *m);
uint32_t chiaro_model_num_triangles(const chiaro_model *m);
uint32_t chiaro_model_num_textures(const chiaro_model *m); /* loaded images */
/* Triangle soup in KDTree order: pos[9n], vnrm[9n] (vertex normals), uv[6n], kd[3n], ke[3n], tex[n]. */
int chiaro_model_triangles(const chiaro_model *m, float *pos, float *vnrm, float *uv, float *kd, float *ke,
                           int32_t *tex);
int chiaro_model_texture(const chiaro_model *m, uint32_t i, int32_t *w, int32_t *h, int32_t *nc,
                         const uint8_t **data);
void chiaro_model_destroy(chiaro_model *m);

/* KDTree without a device (host build only): for kd dumps and for callers that
 * drive libchiaro_hip.so themselves.  Appends to the scene's lightTriangles. */
chiaro_kdtree *chiaro_kdtree_create(chiaro_model *m, chiaro_scene *s, int threads);
uint32_t chiaro_kdtree_num_nodes(const chiaro_kdtree *k);
uint32_t chiaro_kdtree_num_refs(const chiaro_kdtree *k);
int chiaro_kdtree_export(const chiaro_kdtree *k, uint32_t *is_leaf, uint32_t *axis, float *split, uint32_t *child,
                         uint32_t *leaf_first, uint32_t *leaf_count, uint32_t *refs, float *box);
/* Fill the C-ABI scene description (pointers valid while k and s live). */
int chiaro_kdtree_describe(chiaro_kdtree *k, const chiaro_scene *s, cr_scene_desc *out);
void chiaro_kdtree_destroy(chiaro_kdtree *k);

chiaro_raytracer *chiaro_raytracer_create(chiaro_model *m, chiaro_scene *s, int device);
int chiaro_raytracer_raytrace(chiaro_raytracer *r, const float eye[3], const float center[3], const float up[3],
                              float yview);
/* n rayTrace calls with the same view (RayTracer::rayTraceLayers), rendered in pass groups -- on one
 * GPU (cr_render_layers) or across the `gpus` group (cr_group_render_layers); bit-identical. */
int chiaro_raytracer_raytrace_layers(chiaro_raytracer *r, uint32_t n, const float eye[3], const float center[3],
                                     const float up[3], float yview);
/* RayTracer::rayTraceUntil: rayTrace calls with the same view (the accumulation of src/rayTracer.cpp:18-33,59-64)
 * until at most max_above pixels have a relative error above threshold or the frame holds max_layers layers;
 * the noise is checked after each pass group of at most check_every layers (cr_render_until, include/chiaro_hip.h
 * "noise estimate"; floor > 0 is added to the brightness the error is relative to, 1e-3 a usual value).
 * *layer_out (may be NULL): the layer reached.  One GPU only (the `gpus` key above 1: an error).
 * chiaro_raytracer_noise: the statistic of the last check; chiaro_raytracer_noise_map: the error map
 * [yres][xres] of that frame.  chiaro_noise_struct_sizes: sizeof cr_noise_params / cr_noise_stats as this
 * library was built. */
int chiaro_raytracer_raytrace_until(chiaro_raytracer *r, float threshold, uint32_t max_layers, const float eye[3],
                                    const float center[3], const float up[3], float yview, float floor,
                                    uint32_t check_every, uint64_t max_above, uint32_t *layer_out);
int chiaro_raytracer_noise(const chiaro_raytracer *r, cr_noise_stats *out);
int chiaro_raytracer_noise_map(chiaro_raytracer *r, float *err_out);
void chiaro_noise_struct_sizes(uint32_t *params_bytes, uint32_t *stats_bytes);
/* RayTracer::rayTraceAdaptive: the view rendered from layer 1 with further layers -- at most max_layers per pixel,
 * the noise checked every check_every layers from min_layers on -- spent only on the pixels whose relative error is
 * still above threshold (cr_render_adaptive, include/chiaro_hip.h "adaptive sampling"; a pixel at or below it is
 * frozen for good, min_layers guards against freezing on too few samples).  *pixel_layers_out (may be NULL): the
 * pixel-layers rendered, of xres * yres * max_layers.  The frame is then no progressive state: the next raytrace
 * call starts at layer 1 and chiaro_raytracer_checkpoint refuses it.  One GPU only.
 * chiaro_raytracer_adaptive: the statistic of that render; chiaro_raytracer_layer_map: each pixel's layer count,
 * uint32 [yres][xres] (CR_E_INVALID before the first adaptive render). */
int chiaro_raytracer_raytrace_adaptive(chiaro_raytracer *r, float threshold, uint32_t max_layers, const float eye[3],
                                       const float center[3], const float up[3], float yview, float floor,
                                       uint32_t min_layers, uint32_t check_every, uint64_t *pixel_layers_out);
int chiaro_raytracer_adaptive(const chiaro_raytracer *r, cr_adaptive_stats *out);
int chiaro_raytracer_layer_map(const chiaro_raytracer *r, uint32_t *layers_out);
/* RayTracer::denoise: the variance-guided a-trous filter (cr_denoise, include/chiaro_hip.h "guide buffers and
 * denoiser") over the frame of the last chiaro_raytracer_raytrace_until / _raytrace_adaptive (whose layer map it
 * then uses).  chiaro_raytracer_data / _normalize / _export act on the denoised frame until the next raytrace call;
 * chiaro_raytracer_pixels stays the rendered frame, and the progressive state is untouched.  CR_E_HIP with
 * chiaro_last_error when the frame's moments are not complete (any other render) or with gpus > 1.
 * chiaro_raytracer_denoised: the denoised frame [yres][xres][3], NULL when there is none. */
int chiaro_raytracer_denoise(chiaro_raytracer *r, uint32_t levels, float sigma_l, float sigma_z, float sigma_a,
                             uint32_t normal_squarings);
const float *chiaro_raytracer_denoised(const chiaro_raytracer *r);
/* RayTracer::rayTraceTemporal: `layers` layers at this view merged with the history the earlier calls left, carried
 * to this camera through each pixel's first hit (cr_render_temporal, include/chiaro_hip.h "temporal reprojection");
 * the seed advances by one per call.  denoise_levels > 0: the shown frame is filtered with that many a-trous levels.
 * chiaro_raytracer_data / _normalize / _export / _denoised act on the result until the next raytrace call, which
 * starts at layer 1.  *min_count_out (may be NULL): the smallest non-zero sample count of the frame.  One GPU only.
 * chiaro_raytracer_reset_temporal drops the history; chiaro_raytracer_count_map: each pixel's sample count, uint32
 * [yres][xres] (CR_E_INVALID before the first temporal render). */
int chiaro_raytracer_raytrace_temporal(chiaro_raytracer *r, const float eye[3], const float center[3],
                                       const float up[3], float yview, uint32_t layers, uint32_t denoise_levels,
                                       uint32_t *min_count_out);
int chiaro_raytracer_reset_temporal(chiaro_raytracer *r);
int chiaro_raytracer_count_map(const chiaro_raytracer *r, uint32_t *counts_out);
/* RayTracer::radiance / RayTracer::gather (cr_radiance / cr_gather, include/chiaro_hip.h "radiance queries"): the
 * path-traced light along n caller rays (orig, dir: [n][3], dir not normalised), or the mean incoming radiance under
 * the cosine density at n surface points (pos, nrm: [n][3]; irradiance is pi times it; offsetting pos off the surface
 * is the caller's job).  Layers 1 .. layers with the Scene's samples, k, background and seed; ray i draws from the
 * stream of pixel index i.  out [n][3].  The frame, the progressive state and the temporal history are untouched.
 * CR_E_INVALID for a null pointer or layers == 0; CR_E_HIP with chiaro_last_error otherwise.  One GPU only. */
int chiaro_raytracer_radiance(chiaro_raytracer *r, const float *orig, const float *dir, uint32_t n, uint32_t layers,
                              float *out);
int chiaro_raytracer_gather(chiaro_raytracer *r, const float *pos, const float *nrm, uint32_t n, uint32_t layers,
                            float *out);
/* RayTracer::bakeProbes / RayTracer::sampleProbes (cr_probe_sh / cr_probe_sample, include/chiaro_hip.h "probes").
 * _probes: the order-2 SH projection of the light arriving at the probes of `grid` in index order or, with grid null,
 * at the n points pos [n][3]; sh_out [probes][27] = sh[i][k][c].  Layers 1 .. layers with the Scene's samples, k,
 * background and seed; probe i draws from the stream of pixel index i.  _probes_sample: the mean incoming radiance
 * under the cosine density (irradiance / pi, what _gather returns) at m points (pos, nrm: [m][3]) from the grid's
 * coefficients sh, trilinearly interpolated, no visibility weighting; out [m][3].  The frame, the progressive state
 * and the temporal history are untouched.  CR_E_INVALID for a null pointer or layers == 0; CR_E_HIP with
 * chiaro_last_error otherwise.  One GPU only. */
int chiaro_raytracer_probes(chiaro_raytracer *r, const cr_probe_grid *grid /* may be null */, const float *pos,
                            uint32_t n, uint32_t layers, float *sh_out);
int chiaro_raytracer_probes_sample(chiaro_raytracer *r, const cr_probe_grid *grid, const float *sh, const float *pos,
                                   const float *nrm, uint32_t m, float *out);
/* RayTracer::bakeLightmap (cr_bake, include/chiaro_hip.h "lightmap baking"): the width x height lightmap over the
 * lightmap UVs uv ([triangles][6] in the scene's triangle order; null: the grid atlas of the scene's triangles at the
 * largest cell that fits, gutter 0.25, in the map's top-left corner) -- the mean incoming radiance under the cosine
 * density at each covered texel (times pi and the albedo: the caller's), texel y * width + x on the stream of pixel
 * index y * width + x, with the Scene's samples, k, background and seed.  lightmap_out [height][width][3];
 * dilated_out (may be null) the map after `dilate` gutter-filling passes.  _bake renders `layers` layers for every
 * covered texel; _bake_adaptive further layers only where the error is above threshold (the parameters of
 * chiaro_raytracer_raytrace_adaptive), layers_out [height][width] (may be null) the layers each texel holds.
 * CR_E_INVALID for a null handle or output, a zero size or no layers; CR_E_HIP with chiaro_last_error otherwise.
 * One GPU only. */
int chiaro_raytracer_bake(chiaro_raytracer *r, uint32_t width, uint32_t height, const float *uv, uint32_t layers,
                          uint32_t dilate, float *lightmap_out, float *dilated_out);
int chiaro_raytracer_bake_adaptive(chiaro_raytracer *r, uint32_t width, uint32_t height, const float *uv,
                                   float threshold, uint32_t max_layers, float floor, uint32_t min_layers,
                                   uint32_t check_every, uint32_t dilate, float *lightmap_out, float *dilated_out,
                                   uint32_t *layers_out);
const float *chiaro_raytracer_pixels(const chiaro_raytracer *r);
const uint8_t *chiaro_raytracer_data(chiaro_raytracer *r);
float chiaro_raytracer_maxval(const chiaro_raytracer *r);
uint32_t chiaro_raytracer_layers(const chiaro_raytracer *r);
int chiaro_raytracer_counters(const chiaro_raytracer *r, cr_counters *out);
int chiaro_raytracer_normalize(chiaro_raytracer *r, float exposure, float defog, float knee_low, float knee_high,
                               float gamma);
int chiaro_raytracer_export(chiaro_raytracer *r, const char *filename);
cr_ctx *chiaro_raytracer_ctx(chiaro_raytracer *r);

/* Checkpoint / resume of a progressive render (the persisted counterpart of
 * src/rayTracer.cpp:18-33,64 -- layer count, last camera, running average).
 * A resumed RayTracer continues the layers where the checkpoint left them: the next
 * rayTrace at the same camera renders layer `layers + 1` and blends it into the saved
 * average, bit for bit as if the process had never stopped.  A checkpoint of another
 * frame size / spp / depth / seed / background / scene is refused (CR_E_INVALID). */
typedef struct {
    uint32_t xres, yres, samples, k, seed, layers;
    float eye[3], center[3], up[3], yview;
    float background[3];
    uint64_t scene; /* chiaro_kdtree_fingerprint of the scene the average belongs to */
} chiaro_checkpoint;
int chiaro_raytracer_checkpoint(chiaro_raytracer *r, const char *path);
int chiaro_raytracer_resume(chiaro_raytracer *r, const char *path);
uint64_t chiaro_kdtree_fingerprint(const chiaro_kdtree *k);
/* the file format itself (for a caller keeping its own frame, e.g. the multi-GPU
 * DistributedFrame): pixels [yres][xres][3]; read with pixels NULL = header only */
int chiaro_checkpoint_write(const char *path, const chiaro_checkpoint *h, const float *pixels);
int chiaro_checkpoint_read(const char *path, chiaro_checkpoint *h, float *pixels);
void chiaro_raytracer_destroy(chiaro_raytracer *r);

/* OpenEXR as the reference's exportImage writes it (FreeImage_Save(FIF_EXR, FIT_RGBF, 0),
 * src/rayTracer.cpp:229-272): channels B, G, R of HALF, PIZ compression, increasing-Y lines.
 * rgb [H][W][3] (R, G, B; row 0 = top); floats are rounded to half (nearest even, overflow to
 * infinity).  chiaro_exr_read_half reads scanline HALF R/G/B files with NO or PIZ compression;
 * with rgb NULL it returns the size only; cap = halves available at rgb. */
int chiaro_exr_write(const char *path, const float *rgb, uint32_t w, uint32_t h);
int chiaro_exr_write_half(const char *path, const uint16_t *rgb, uint32_t w, uint32_t h);
int chiaro_exr_read_half(const char *path, uint32_t *w, uint32_t *h, uint16_t *rgb, size_t cap);
int chiaro_float_to_half(const float *in, uint16_t *out, size_t n);

int chiaro_camera(const float eye[3], const float center[3], const float up[3], float yview, uint32_t xres,
                  uint32_t yres, cr_camera *out);

/* Headless preview session over a RayTracer (and its Scene: exposure keys change it). */
typedef struct chiaro_preview chiaro_preview;
enum {
    CHIARO_KEY_R = 0,     /* render a layer at the camera, show it            */
    CHIARO_KEY_TAB = 1,   /* toggle render / model view                        */
    CHIARO_KEY_EQUAL = 2, /* exposure + 0.2, re-normalise                      */
    CHIARO_KEY_MINUS = 3, /* exposure - 0.2, re-normalise                      */
    CHIARO_KEY_W = 4, CHIARO_KEY_S = 5, CHIARO_KEY_A = 6, CHIARO_KEY_D = 7, CHIARO_KEY_E = 8, CHIARO_KEY_Q = 9,
    /* a frame without a movement key: only the shift state (the speed of the next move) */
    CHIARO_KEY_SHIFT = 10
};
chiaro_preview *chiaro_preview_create(chiaro_scene *s, chiaro_raytracer *r);
/* one key press; dt = frame time for the movement keys, shift = LEFT_SHIFT held */
int chiaro_preview_key(chiaro_preview *p, int key, float dt, int shift);
/* on != 0: key R renders through chiaro_raytracer_raytrace_temporal, so a moved camera keeps the samples taken so far
 * instead of restarting at layer 1; 0 (the default): the reference's behaviour.  A change drops the history. */
int chiaro_preview_set_temporal(chiaro_preview *p, int on);
int chiaro_preview_mouse(chiaro_preview *p, float xoffset, float yoffset);
int chiaro_preview_scroll(chiaro_preview *p, float yoffset);
/* the screen texture (RayTracer::getData after normalizeImage), width x height x RGB8 */
const uint8_t *chiaro_preview_texture(chiaro_preview *p, uint32_t *width, uint32_t *height);
/* camera Position, Front, Up, Zoom (degrees); show_render, renders so far */
int chiaro_preview_state(const chiaro_preview *p, float position[3], float front[3], float up[3], float *zoom,
                         int *show_render, uint32_t *renders);
void chiaro_preview_destroy(chiaro_preview *p);
/* The preview camera alone (no GPU): Camera(VP, LA, UP) with Zoom from yview, then
 * nops operations -- op 0..5 ProcessKeyboard(FORWARD..DOWNWARD, dt = a0), 6
 * ProcessMouseMovement(a0, a1), 7 ProcessMouseScroll(a0), 8 MovementSpeed = a0
 * (args: 2 per op) -- and after each: Position, Front, Up, Right, Yaw, Pitch, Zoom
 * (15 floats per op) into out.  A GL-free front-end can plan camera paths with it. */
int chiaro_preview_camera_replay(const float vp[3], const float la[3], const float up[3], float yview,
                                 const int32_t *ops, const float *args, int nops, float *out);

#ifdef __cplusplus
}
#endif
#endif
