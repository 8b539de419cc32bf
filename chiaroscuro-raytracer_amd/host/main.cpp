// main.cpp -- offline front-end, the counterpart of the reference's main.cpp:5-21
// with the render loop on the MI355X:
//
//   bin/chiaroscuro scene.rtc [rtc tokens...]
//
// Scene(argc, argv) -> Model(scene) -> RayTracer(model, scene) ->
// rayTrace(VP, LA, UP, yview) -> exportImage(renderPath), as the reference's
// offline branch.  The OpenGL preview is not part of this build:
// with "preview" enabled in the .rtc the scene is rendered offline instead.
// Extra token "layers N" (this build): render N progressive layers of the same
// view (the reference's preview accumulates them the same way,
// src/rayTracer.cpp:17-33, src/openglPreview.cpp:247-255).
// Extra token "noise T" (this build): render until no pixel's relative error exceeds T
// (RayTracer::rayTraceUntil); N of "layers N" is then the most layers to render.
// Extra token "adaptive T" (this build): further layers only for the pixels whose relative error exceeds T
// (RayTracer::rayTraceAdaptive); N of "layers N" is then the most layers of any pixel.
// Extra token "denoise N" (this build, with "noise T" or "adaptive T" only -- the renders that keep the frame's
// moments): the frame is filtered with N a-trous levels (RayTracer::denoise) before it is exported.
#include "model.hpp"
#include "raytracer.hpp"
#include "scene.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

int main(int argc, char **argv) {
    // strip this build's own tokens before Scene sees them
    unsigned layers = 1;
    float noise = -1.f;    // "noise T": T >= 0
    float adaptive = -1.f; // "adaptive T": T >= 0
    int denoise = -1;      // "denoise N": 0 <= N <= 8 levels
    std::vector<char *> args;
    for (int i = 0; i < argc; i++) {
        if (i > 1 && !std::strcmp(argv[i], "layers") && i + 1 < argc) {
            layers = (unsigned)std::max(1, std::atoi(argv[++i]));
            continue;
        }
        if (i > 1 && !std::strcmp(argv[i], "noise") && i + 1 < argc) {
            noise = (float)std::atof(argv[++i]);
            if (!(noise >= 0.f)) {
                std::fprintf(stderr, "chiaroscuro: noise takes a threshold >= 0\n");
                return 1;
            }
            continue;
        }
        if (i > 1 && !std::strcmp(argv[i], "adaptive") && i + 1 < argc) {
            adaptive = (float)std::atof(argv[++i]);
            if (!(adaptive >= 0.f)) {
                std::fprintf(stderr, "chiaroscuro: adaptive takes a threshold >= 0\n");
                return 1;
            }
            continue;
        }
        if (i > 1 && !std::strcmp(argv[i], "denoise") && i + 1 < argc) {
            char *end = nullptr;
            const long n = std::strtol(argv[++i], &end, 10);
            if (end == argv[i] || *end || n < 0 || n > 8) {
                std::fprintf(stderr, "chiaroscuro: denoise takes a number of levels, 0..8\n");
                return 1;
            }
            denoise = (int)n;
            continue;
        }
        args.push_back(argv[i]);
    }
    if (denoise >= 0 && noise < 0.f && adaptive < 0.f) {
        std::fprintf(stderr, "chiaroscuro: denoise needs the frame's moments: use it with noise T or adaptive T\n");
        return 1;
    }
    try {
        chiaro::Scene scene((int)args.size(), args.data());
        if (scene.usingOpenGLPreview)
            std::fprintf(stderr, "chiaroscuro: OpenGL preview not built; rendering offline (add no-preview)\n");
        chiaro::Model model(scene);
        if (!model.error.empty()) std::fprintf(stderr, "%s\n", model.error.c_str());
        chiaro::RayTracer renderer(model, scene);
        // the layers in pass groups (RayTracer::rayTraceLayers, bit-identical to one rayTrace per layer)
        if (adaptive >= 0.f && noise >= 0.f) {
            std::fprintf(stderr, "chiaroscuro: noise and adaptive exclude each other\n");
            return 1;
        }
        if (adaptive >= 0.f) {
            const unsigned long long done =
                renderer.rayTraceAdaptive(adaptive, layers, scene.VP, scene.LA, scene.UP, scene.yview);
            const cr_adaptive_stats &st = renderer.lastAdaptive();
            std::fprintf(stderr, "adaptive %g: %llu of %llu pixel-layers rendered, %u checks, %llu pixels still above, "
                                 "max error %g\n",
                         adaptive, done, (unsigned long long)st.pixels * layers, st.checks,
                         (unsigned long long)st.active, st.max_err);
        } else if (noise >= 0.f) {
            const unsigned reached = renderer.rayTraceUntil(noise, layers, scene.VP, scene.LA, scene.UP, scene.yview);
            const cr_noise_stats &st = renderer.lastNoise();
            std::fprintf(stderr, "noise %g: layer %u of at most %u reached, %llu of %llu pixels above, max error %g (%s)\n",
                         noise, reached, layers, (unsigned long long)st.above, (unsigned long long)st.pixels,
                         st.max_err, st.above == 0 ? "converged" : "not converged");
        } else
            renderer.rayTraceLayers(layers, scene.VP, scene.LA, scene.UP, scene.yview);
        std::fprintf(stderr, "layers 1..%u: %.3f s, %llu rays\n", renderer.layers(), renderer.lastSeconds(),
                     (unsigned long long)(renderer.lastCounters().closest + renderer.lastCounters().shadow));
        if (denoise >= 0) {
            renderer.denoise((unsigned)denoise);
            std::fprintf(stderr, "denoise %d: %d a-trous level(s) over %u layer(s) x %u spp%s\n", denoise, denoise,
                         renderer.layers(), scene.samples, adaptive >= 0.f ? ", per-pixel layer map" : "");
        }
        renderer.exportImage(scene.renderPath.c_str());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "chiaroscuro: %s\n", e.what());
        return 1;
    }
    return 0;
}
