// p3d_render -- command-line front end: the offline branch of the reference's main()
// (RT/main.cpp:949-976: init_scene -> renderScene -> save image) on an MI355X.
//   p3d_render <scene.p3f> [--res W H] [--accel 0|1|2] [--depth D] [--spp N] [--seed S]
//              [--device K | --gpus N] [--out image.png|image.ppm] [--counters] [--soft-shadow] [--fuzzy-reflection]
//              [--aov PREFIX] [--denoise K [--denoise-sigmas Z A C]] [--accumulate [--accumulate-params TOL NMIN MAXLEN]]
//              [--variance-guided [--variance-params MIN_TEMPORAL RADIUS SIGMA]] [--ao S RADIUS [--ao-scale F] [--ao-out PREFIX]]
//              [--gi S [--gi-bias B] [--gi-bounces B]]
// --gpus N: devices 0..N-1 each render every N-th block of 16 rows, one RCCL gather to device 0.
// --orbit N STEP_DEG: N frames of the reference's mouse orbit (alpha advancing by STEP_DEG per frame, RT/main.cpp:339-341,
// 419-421) in ONE p3d_render_frames call; --out then takes a %d pattern (e.g. frame_%03d.png) for the frame number.
// --aov PREFIX: also writes the primary hits' depth, normal and albedo planes (p3d_render_aov) as float32 NumPy files
// PREFIX_depth.npy (H, W), PREFIX_normal.npy and PREFIX_albedo.npy (H, W, 3), bottom row first like img_Data.
// --denoise K: the frame is filtered by p3d_denoise (K passes, 0..6) before it is written to --out; --denoise-sigmas Z A C sets
// sigma_depth, sigma_albedo and sigma_color (C = 0: no colour stop).  Combines with --aov, --soft-shadow, --fuzzy-reflection and
// --spp; one frame on one GPU: not with --orbit (but see --accumulate), and not with --gpus N (a rank's shard is not a frame).
// --orbit N STEP --accumulate: the orbit's frames are a sequence -- each is blended with the history reprojected from the
// frame before it (p3d_accumulate) before it is written; --accumulate-params TOL NMIN MAXLEN sets depth_tolerance,
// normal_min and max_history.  With it --denoise K is legal together with --orbit and filters every accumulated frame (one
// p3d_denoise call over all N).  One GPU; needs --orbit.
// --orbit N STEP --accumulate --denoise K --variance-guided: the accumulation also carries the luminance moments of every
// pixel (p3d_accumulate_variance over the sequence) and the filter is steered by their variance (p3d_denoise_variance, one
// call over all N); --variance-params MIN_TEMPORAL RADIUS SIGMA sets the history below which the variance is estimated from
// the neighbours, that neighbourhood's radius (1..3) and the colour stop's width in standard deviations.  Needs both
// --accumulate and --denoise.
// --ao S RADIUS: the frame is rendered with its planes, p3d_ambient_occlusion runs S (1, 2, 4, .. 64) segments of length RADIUS
// per pixel over them and the colour is multiplied by the result before it is written.  Combines with --denoise K (the
// modulated colour is what is filtered), with --aov and with --orbit N STEP [--accumulate]; one GPU: not with --gpus N.
// --ao-out PREFIX also writes the plane as PREFIX_ao.npy (H, W) (with --orbit: PREFIX_ao_<frame>.npy).
// --ao S RADIUS --ao-scale F: the occlusion is computed at 1 / F of the resolution (F in 1..4, dividing W and H; 1: as without)
// on planes rendered at that resolution and brought up along the frame's own depth and normal by p3d_upsample; everything
// after it (the modulation, --ao-out, --denoise, --accumulate) sees the upsampled plane.
// --gi S [--gi-bias B]: the frame is rendered with its planes, p3d_indirect_diffuse gathers one bounce of diffuse indirect
// light with S (1, 2, 4, .. 64) rays per pixel over them (origins moved B along the normal, default 0.001) and
// albedo * indirect is added to the colour before it is written.  Combines with --denoise K (the sum is what is filtered),
// with --ao (applied first) and with --aov; one frame on one GPU: not with --orbit, not with --gpus N.
// --gi S --gi-bounces B: p3d_indirect_paths in its place, S paths per pixel of at most B (1 .. 8) rays each; needs --gi.
// Defaults are the reference's: resolution / accel / spp from the file, MAX_DEPTH 4.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../host/p3d_scene.h"

using namespace p3d_host;

static int save_ppm(const char* path, const std::vector<uint8_t>& img, int w, int h) {
    FILE* f = fopen(path, "wb");
    if (!f) return -1;
    fprintf(f, "P6\n%d %d\n255\n", w, h);
    for (int y = h - 1; y >= 0; y--)                 // img_Data is bottom row first
        fwrite(img.data() + (size_t)y * w * 3, 1, (size_t)w * 3, f);
    fclose(f);
    return 0;
}

// NumPy .npy, format 1.0: magic, version, a little-endian header length, a Python dict padded with spaces to a multiple of
// 64 bytes and ended by a newline, then the float32 data in C order.
static int save_npy(const std::string& path, const std::vector<float>& v, int h, int w, int c) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return -1;
    char shape[64];
    if (c > 1) snprintf(shape, sizeof shape, "(%d, %d, %d)", h, w, c); else snprintf(shape, sizeof shape, "(%d, %d)", h, w);
    std::string hdr = std::string("{'descr': '<f4', 'fortran_order': False, 'shape': ") + shape + ", }";
    while ((10 + hdr.size() + 1) % 64) hdr += ' ';
    hdr += '\n';
    const unsigned char pre[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(hdr.size() & 255), (unsigned char)(hdr.size() >> 8)};
    bool ok = fwrite(pre, 1, 10, f) == 10 && fwrite(hdr.data(), 1, hdr.size(), f) == hdr.size() &&
              fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
    return (fclose(f) == 0 && ok) ? 0 : -1;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s scene.p3f [--res W H] [--accel A] [--depth D] [--spp N] [--seed S] "
                        "[--device K | --gpus N] [--out file.ppm] [--orbit N STEP_DEG] [--counters] [--soft-shadow] [--fuzzy-reflection] [--schlick] [--aov PREFIX] "
                        "[--denoise K [--denoise-sigmas Z A C]] [--accumulate [--accumulate-params TOL NMIN MAXLEN]] "
                        "[--variance-guided [--variance-params MIN_TEMPORAL RADIUS SIGMA]] [--ao S RADIUS [--ao-scale F] [--ao-out PREFIX]] [--gi S [--gi-bias B] [--gi-bounces B]]\n"
                        "  --denoise filters one frame on one GPU: not with --orbit, not with --gpus N\n"
                        "  --accumulate blends the frames of --orbit over time on one GPU; with it --denoise filters every accumulated frame\n"
                        "  --variance-guided steers that filter by the variance of every pixel's luminance over time: needs --accumulate and --denoise\n"
                        "  --ao multiplies the colour by ambient occlusion (S segments of length RADIUS per pixel) on one GPU: not with --gpus N\n"
                        "  --ao-scale computes it at 1 / F of the resolution (F in 1..4, dividing W and H) and upsamples it along the frame's depth and normal: needs --ao\n"
                        "  --gi adds one bounce of diffuse indirect light (S rays per pixel) to one frame on one GPU: not with --orbit, not with --gpus N\n"
                        "  --gi-bounces follows every ray of --gi over up to B (1..8) diffuse bounces: needs --gi\n", argv[0]);
        return 2;
    }
    RenderOptions opt;
    int rw = 0, rh = 0, orbit_n = 0;
    float orbit_step = 0.0f;
    std::string out = "RT_Output.png";                       // the reference's file name, RT/main.cpp:968
    std::string aov;                                         // --aov PREFIX
    std::string ao_out;                                      // --ao-out PREFIX
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i];
        auto need = [&](int n) { if (i + n >= argc) { fprintf(stderr, "%s needs %d value(s)\n", a.c_str(), n); exit(2); } };
        if (a == "--res") { need(2); rw = atoi(argv[++i]); rh = atoi(argv[++i]); }
        else if (a == "--accel") { need(1); opt.accel = atoi(argv[++i]); }
        else if (a == "--depth") { need(1); opt.max_depth = atoi(argv[++i]); }
        else if (a == "--spp") { need(1); opt.spp = atoi(argv[++i]); }
        else if (a == "--seed") { need(1); opt.seed = (unsigned)strtoul(argv[++i], nullptr, 10); }
        else if (a == "--device") { need(1); opt.device = atoi(argv[++i]); }
        else if (a == "--gpus") { need(1); opt.gpus = atoi(argv[++i]); }
        else if (a == "--out") { need(1); out = argv[++i]; }
        else if (a == "--orbit") { need(2); orbit_n = atoi(argv[++i]); orbit_step = (float)atof(argv[++i]); if (orbit_n < 1) { fprintf(stderr, "--orbit needs N >= 1\n"); return 2; } }
        else if (a == "--counters") opt.counters = true;
        else if (a == "--soft-shadow") opt.SOFT_SHADOW = true;
        else if (a == "--fuzzy-reflection") opt.FUZZY_REFLECTION = true;
        else if (a == "--schlick") opt.SCHLICK_APPROX = true;
        else if (a == "--aov") { need(1); aov = argv[++i]; opt.want_aov = true; }
        else if (a == "--denoise") { need(1); opt.denoise = atoi(argv[++i]); if (opt.denoise < 0 || opt.denoise > 6) { fprintf(stderr, "--denoise needs K in 0..6\n"); return 2; } }
        else if (a == "--denoise-sigmas") { need(3); opt.denoise_sigma_depth = (float)atof(argv[++i]); opt.denoise_sigma_albedo = (float)atof(argv[++i]); opt.denoise_sigma_color = (float)atof(argv[++i]); }
        else if (a == "--accumulate") opt.accumulate = true;
        else if (a == "--variance-guided") opt.variance_guided = true;
        else if (a == "--variance-params") { need(3); opt.variance_min_temporal = (float)atof(argv[++i]); opt.variance_radius = atoi(argv[++i]); opt.variance_sigma_color = (float)atof(argv[++i]); }
        else if (a == "--accumulate-params") { need(3); opt.accumulate_depth_tolerance = (float)atof(argv[++i]); opt.accumulate_normal_min = (float)atof(argv[++i]); opt.accumulate_max_history = (float)atof(argv[++i]); }
        else if (a == "--ao") {
            need(2); opt.ambient_occlusion = atoi(argv[++i]); opt.ao_radius = (float)atof(argv[++i]);
            const int S = opt.ambient_occlusion;
            if (S < 1 || S > 64 || (S & (S - 1)) || !(opt.ao_radius > 0.0f)) { fprintf(stderr, "--ao needs S in 1, 2, 4, .. 64 and RADIUS > 0\n"); return 2; }
        }
        else if (a == "--ao-out") { need(1); ao_out = argv[++i]; }
        else if (a == "--ao-scale") { need(1); opt.ao_scale = atoi(argv[++i]); if (opt.ao_scale < 1 || opt.ao_scale > 4) { fprintf(stderr, "--ao-scale needs F in 1..4\n"); return 2; } }
        else if (a == "--gi") {
            need(1); opt.indirect_diffuse = atoi(argv[++i]);
            const int S = opt.indirect_diffuse;
            if (S < 1 || S > 64 || (S & (S - 1))) { fprintf(stderr, "--gi needs S in 1, 2, 4, .. 64\n"); return 2; }
        }
        else if (a == "--gi-bias") { need(1); opt.indirect_bias = (float)atof(argv[++i]); if (!(opt.indirect_bias >= 0.0f)) { fprintf(stderr, "--gi-bias needs B >= 0\n"); return 2; } }
        else if (a == "--gi-bounces") { need(1); opt.indirect_bounces = atoi(argv[++i]); if (opt.indirect_bounces < 1 || opt.indirect_bounces > 8) { fprintf(stderr, "--gi-bounces needs B in 1..8\n"); return 2; } }
        else { fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    Scene scene;
    if (!scene.load_p3f(argv[1])) { fprintf(stderr, "Error opening P3F file: %s\n", scene.parse_error().c_str()); return 1; }
    if (rw > 0 && rh > 0) scene.GetCamera()->SetResolution(rw, rh);
    printf("Scene loaded: %d objects, %d lights, %dx%d\n", scene.getNumObjects(), scene.getNumLights(),
           scene.GetCamera()->GetResX(), scene.GetCamera()->GetResY());
    const int W = scene.GetCamera()->GetResX(), H = scene.GetCamera()->GetResY();
    auto save = [&](const std::string& path, const uint8_t* img) {
        const bool ppm = path.size() > 4 && path.compare(path.size() - 4, 4, ".ppm") == 0;
        if (ppm) { std::vector<uint8_t> v(img, img + (size_t)W * H * 3); return save_ppm(path.c_str(), v, W, H); }
        return save_png(path.c_str(), img, W, H);
    };
    if (orbit_n > 0 && opt.want_aov) { fprintf(stderr, "--aov writes the planes of one frame: not with --orbit\n"); return 2; }
    if (opt.accumulate && (orbit_n < 1 || opt.gpus > 1)) { fprintf(stderr, "--accumulate blends the frames of --orbit N STEP on one GPU: it needs --orbit, not --gpus N\n"); return 2; }
    if (opt.variance_guided && (!opt.accumulate || opt.denoise < 0)) { fprintf(stderr, "--variance-guided steers the filter of an accumulated sequence: it needs --accumulate and --denoise K\n"); return 2; }
    if (opt.ambient_occlusion > 0 && opt.gpus > 1) { fprintf(stderr, "--ao runs on the planes of whole frames on one GPU: not with --gpus N\n"); return 2; }
    if (opt.indirect_diffuse > 0 && (opt.gpus > 1 || orbit_n > 0)) { fprintf(stderr, "--gi gathers over the planes of one whole frame on one GPU: not with --gpus N or --orbit\n"); return 2; }
    if (opt.indirect_bounces > 0 && opt.indirect_diffuse < 1) { fprintf(stderr, "--gi-bounces needs --gi S\n"); return 2; }
    if (opt.ao_scale != 1 && opt.ambient_occlusion < 1) { fprintf(stderr, "--ao-scale needs --ao S RADIUS\n"); return 2; }
    if (W % opt.ao_scale || H % opt.ao_scale) { fprintf(stderr, "--ao-scale F must divide both resolutions (%d x %d)\n", W, H); return 2; }
    if (!ao_out.empty() && opt.ambient_occlusion < 1) { fprintf(stderr, "--ao-out needs --ao S RADIUS\n"); return 2; }
    if (opt.denoise >= 0 && ((orbit_n > 0 && !opt.accumulate) || opt.gpus > 1)) { fprintf(stderr, "--denoise filters one frame on one GPU: not with --orbit or --gpus N\n"); return 2; }
    if (orbit_n > 0) {
        {   // exactly one conversion, %d or %0Nd: the pattern is handed to snprintf
            const size_t pc = out.find('%');
            size_t e = pc == std::string::npos ? pc : out.find_first_not_of("0123456789", pc + 1);
            if (pc == std::string::npos || e == std::string::npos || out[e] != 'd' || out.find('%', pc + 1) != std::string::npos) {
                fprintf(stderr, "--orbit needs an --out pattern with one %%d (e.g. frame_%%03d.png)\n");
                return 2;
            }
        }
        const std::vector<Vector> eyes = orbit_eyes(scene.GetCamera()->GetEye(), orbit_n, orbit_step, 0.0f);
        RenderResult res;
        std::string err;
        int rc = renderFrames(scene, opt, eyes, false, false, res, &err);
        if (rc) { fprintf(stderr, "render failed (%d): %s\n", rc, err.c_str()); return 1; }
        printf("Done: %d frames, %.4f ms per frame on the device stream\n", orbit_n, res.kernel_ms / orbit_n);
        for (int f = 0; f < orbit_n; f++) {
            char path[4096];
            snprintf(path, sizeof path, out.c_str(), f);
            if (save(path, res.img_Data.data() + (size_t)f * W * H * 3)) { fprintf(stderr, "Error saving Image file\n"); return 1; }
            printf("Image file created: %s\n", path);
            if (!ao_out.empty()) {
                const std::vector<float> plane(res.ao.begin() + (size_t)f * W * H, res.ao.begin() + (size_t)(f + 1) * W * H);
                const std::string npy = ao_out + "_ao_" + std::to_string(f) + ".npy";
                if (save_npy(npy, plane, H, W, 1)) { fprintf(stderr, "Error saving %s\n", npy.c_str()); return 1; }
            }
        }
        return 0;
    }
    RenderResult res;
    std::string err;
    auto t0 = std::chrono::high_resolution_clock::now();
    int rc = renderScene(scene, opt, false, false, res, &err);
    auto t1 = std::chrono::high_resolution_clock::now();
    if (rc) { fprintf(stderr, "render failed (%d): %s\n", rc, err.c_str()); return 1; }
    printf("Done: %.3f ms on the device stream, %.3f s wall incl. BVH build and upload\n", res.kernel_ms,
           std::chrono::duration<double>(t1 - t0).count());
    if (opt.counters) {
        unsigned long long rays = res.counters.closest_queries + res.counters.shadow_queries;
        printf("rays=%llu (closest %llu, shadow %llu) box=%llu sph=%llu tri=%llu\n", rays,
               (unsigned long long)res.counters.closest_queries, (unsigned long long)res.counters.shadow_queries,
               (unsigned long long)res.counters.box_tests, (unsigned long long)res.counters.sphere_tests,
               (unsigned long long)res.counters.tri_tests);
    }
    if (save(out, res.img_Data.data())) {
        fprintf(stderr, "Error saving Image file\n");
        return 1;
    }
    printf("Image file created: %s\n", out.c_str());
    if (!ao_out.empty()) {
        if (save_npy(ao_out + "_ao.npy", res.ao, H, W, 1)) { fprintf(stderr, "Error saving the ambient occlusion file\n"); return 1; }
        printf("Ambient occlusion file created: %s_ao.npy\n", ao_out.c_str());
    }
    if (opt.want_aov) {
        if (save_npy(aov + "_depth.npy", res.depth, H, W, 1) || save_npy(aov + "_normal.npy", res.normal, H, W, 3) ||
            save_npy(aov + "_albedo.npy", res.albedo, H, W, 3)) {
            fprintf(stderr, "Error saving the AOV files\n");
            return 1;
        }
        printf("AOV files created: %s_depth.npy %s_normal.npy %s_albedo.npy\n", aov.c_str(), aov.c_str(), aov.c_str());
    }
    return 0;
}
