// Main.cpp — the rt3 command line: same flags, defaults, messages and exit codes as the reference's entry point
// (src/Main.cpp:62-81 options, :89-239 parsing, :246-315 main), driving the HIP backend through the reference's own
// call sequence: initialize_renderer() -> Camera::update -> create_* -> prerender -> render -> Frame::to_ppm/to_png.
//
// Kept: -f/--format png|ppm (default png), -W/--width (800), -H/--height (600), -h/--help, first positional =
// output path (later ones ignored), value forms `-W 400`, `-W400`, `--width 400`; exit code 0 after help, -1 on a
// usage error, -1 on a fatal backend error.  Fixed: `--key=value`, which the reference mis-parses (Main.cpp:110).
// Added (defaults reproduce the reference render): --scene, --spp, --depth, --seed, --gpus; Mode X only: --aov, --hdr, --denoise (PFM files),
// --frames, --orbit and --slide (a sequence, denoised temporally), --adaptive and --counts (--spp as a budget), --rays and --radiance
// (path-traced radiance along rays read from a file), --env (an environment map from a PFM of six stacked cube faces),
// --env-sampling (importance sampling of that map with shadow rays), --light-sampling (the same for the emissive primitives),
// --display (the image written is the linear frame through exposure, a tone curve and a transfer function), --lens, --lens-fov and
// --lens-extent (the frame of another lens model at the scene's camera position: equirectangular, fisheye, orthographic, cube),
// --lens-frames (a sequence of such frames, denoised temporally through the lens), --display-frames, --adapt and --bloom (an image
// per frame of a sequence through the display transform, an exposure that follows the sequence, a bloom pyramid).
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "renderer/Renderer.hpp"
#include "sceneparser/SceneParser.hpp"

using namespace RayTracer;

namespace {

struct Options {
    std::string output_path;
    bool png = true;
    uint32_t width = 800, height = 600;
    std::string scene = "builtin";
    uint32_t spp = 0, depth = 50, seed = 1, gpus = 1;
    bool gpu_prerender = false, dump_scene = false;
    std::string aov_prefix, hdr_path;                              // Mode X: first-hit AOVs / the linear beauty as PFM files
    bool aov_specular = false;                                     // --aov-specular: --aov and the single-frame --denoise take specular-chain guides
    rt3_aov_chain_params chain{ 0u, 0.0f, 0u, 0u };
    std::string denoise_path;                                      // Mode X: the denoised linear frame as a PFM file
    uint32_t frames = 1;                                           // Mode X: frames of a sequence (frame k renders with seed + k)
    float orbit = 0.0f;                                            // look-at scenes: degrees the look-from point turns per frame
    bool have_orbit = false;
    float slide[3] = { 0.0f, 0.0f, 0.0f };                         // sphere scenes: what every sphere of odd index moves by per frame
    bool have_slide = false;
    bool refit = false;                                            // --slide: frames after the first update the spheres in place (rt3_update_spheres)
    uint32_t regroup = 0;                                          // --refit: every regroup-th refit frame is followed by rt3_regroup (0: never)
    bool have_regroup = false;
    bool adaptive = false;                                         // Mode X: --spp is a budget (rt3_render_path_adaptive)
    float adaptive_threshold = 0.05f;
    uint32_t adaptive_min = 0, adaptive_step = 16;                 // (min 0: not given = min(16, spp))
    std::string counts_path;                                       // --adaptive: the samples per pixel as a 1-channel PFM
    std::string rays_path, radiance_path;                          // Mode X: rt3_ray records in, their radiance out as a PFM of n x 1
    std::string env_path;                                          // Mode X: the environment map, a colour PFM of N x 6N (the six faces stacked)
    bool env_sampling = false;                                     // with --env: RT3_FLAG_ENV_SAMPLING
    bool light_sampling = false;                                   // Mode X: RT3_FLAG_LIGHT_SAMPLING
    struct Texture { std::string path; uint32_t wrap; };           // Mode X, sphere scenes: --texture FILE.pfm[,repeat|clamp], use k fills slot k
    std::vector<Texture> textures;
    struct SphereBind { bool all; uint32_t index, slot; };         // --bind-sphere INDEX=SLOT | all=SLOT, applied in the order given
    std::vector<SphereBind> sphere_binds;
    bool display = false;                                         // Mode X: the image written is rt3_display of the linear (or the denoised) frame
    uint32_t lens = 0;                                             // Mode X: RT3_LENS_* of the frame to render instead of the camera's (0: none)
    float lens_fov = 180.0f;                                       // fisheye: the whole field of view across the shorter image side, in degrees
    float lens_extent[2] = { 2.0f, 2.0f };                         // ortho: the window's width and height
    bool have_lens_fov = false, have_lens_extent = false;
    uint32_t lens_frames = 1;                                      // --lens: frames of a sequence of lens frames (frame k renders with seed + k)
    bool have_lens_frames = false;
    rt3_display_params display_params{ RT3_DISPLAY_FILMIC, RT3_DISPLAY_SRGB, 0u, 102u, 51u, 1.0f, 0.18f, 4.0f };      // the defaults of DESIGN.md 4.22
    std::string display_frames;                                    // with --display and a sequence: PREFIX of one image per frame (rt3_display_sequence)
    bool have_adapt = false, have_bloom = false;
    uint32_t adapt[2] = { 256u, 64u };                             // --adapt: the share of the way to a brighter / darker target per frame, in 1/1024
    uint32_t bloom_levels = 0;                                     // --bloom: the pyramid's levels, the threshold, the intensity
    float bloom_threshold = 1.0f, bloom_intensity = 0.25f;
    rt3_display_sequence_params sequence_params() const {
        return rt3_display_sequence_params{ display_params, adapt[0], adapt[1], bloom_levels, bloom_threshold, bloom_intensity, { 0u, 0u, 0u } };
    }
};

void print_usage(const char* exe) {
    std::cout << "Usage: " << exe << " [<options>] <output_path>\n\n"
              << "Options:\n"
              << "\t-f,--format\tThe format of the resulting frame. Supported formats are: 'png' and 'ppm' (default: png).\n"
              << "\t-W,--width\tThe width of the resulting image, in pixels (default: 800).\n"
              << "\t-H,--height\tThe height of th resulting image, in pixels (default: 600).\n"
              << "\t   --scene\tbuiltin | three | weekend | stress100k | cornell | <file>.scene (default: builtin = src/Main.cpp's teddy + sphere).\n"
              << "\t   --spp\tSamples per pixel; enables the path tracer (default: off = the reference's 1-ray render).\n"
              << "\t   --depth\tMaximum ray casts per path (default: 50).\n"
              << "\t   --seed\tRender seed (default: 1).\n"
              << "\t   --gpus\tNumber of GPUs to shard the frame over (default: 1).\n"
              << "\t   --gpu-prerender\tTessellate spheres on the GPU instead of the host (same arrays).\n"
              << "\t   --dump-scene\tParse the --scene file, print its entities and exit.\n"
              << "\t   --aov-specular\tBOUNCES[,MAX_FUZZ]. Mode X: --aov and the single-frame --denoise take their guides at the first rough surface behind\n"
              << "\t\t\tglass and metals of fuzz <= MAX_FUZZ (default 0), following at most BOUNCES (<= 16) bounces. Not with --frames or --lens-frames.\n"
              << "\t   --aov\tMode X: also write the first-hit AOVs as PREFIX.albedo.pfm, PREFIX.normal.pfm and PREFIX.depth.pfm.\n"
              << "\t   --hdr\tMode X: also write the linear (float) frame to this path as a 3-channel PFM.\n"
              << "\t   --denoise\tMode X: also write the denoised linear frame (a-trous, AOV-guided) to this path as a 3-channel PFM;\n"
              << "\t\t\twith --frames N > 1, write PREFIX.<k>.pfm for every frame k, denoised temporally.\n"
              << "\t   --frames\tMode X: render a sequence of N frames, frame k with seed + k; the image written is the last (default: 1).\n"
              << "\t   --orbit\tweekend / stress100k: turn the look-from point by k * DEG degrees about the vertical axis through the look-at point.\n"
              << "\t   --slide\tthree / weekend / stress100k with --frames: translate every sphere of odd index by k * (DX,DY,DZ) in frame k;\n"
              << "\t\t\twith --denoise PREFIX the temporal filter follows them (the motion plane).\n"
              << "\t   --refit\tWith --slide: frames after the first move the spheres by an update on the device instead of a full upload (same frames).\n"
              << "\t   --regroup\tWith --refit: K: after every K-th refit frame the group order is rebuilt on the device (rt3_regroup; same frames).\n"
              << "\t   --adaptive\tMode X: T[,MIN[,STEP]]: --spp is a budget; MIN samples for every pixel (default: 16), then STEP at a time (default: 16)\n"
              << "\t\t\tfor the pixels whose neighbourhood has not reached a relative standard error of T. Combines with --hdr, --aov, --denoise.\n"
              << "\t   --counts\tWith --adaptive: also write the samples every pixel received to this path as a 1-channel PFM.\n"
              << "\t   --rays\tMode X, with --radiance: a file of raw little-endian rt3_ray records (32 bytes each: origin, t_max = +inf, unit direction, pad).\n"
              << "\t   --radiance\tMode X, with --rays: write the path-traced radiance along those rays (--spp samples per ray, --depth, --seed) to this\n"
              << "\t\t\tpath as a 3-channel PFM, n wide and 1 high.\n"
              << "\t   --env\tMode X: light the scene with a cube map where a ray leaves it: a colour PFM, N wide and 6N high, the faces +X, -X, +Y, -Y,\n"
              << "\t\t\t+Z, -Z stacked from top to bottom, N up to 2048. The render, --radiance and --aov use it.\n"
              << "\t   --env-sampling\tWith --env: every diffuse bounce also samples the map by its brightness and casts one shadow ray (a small bright\n"
              << "\t\t\tsun converges). The render and --radiance; not with --adaptive, nor with a scene whose background is black.\n"
              << "\t   --light-sampling\tMode X: every diffuse bounce also samples the emissive primitives by brightness times area and casts one shadow\n"
              << "\t\t\tray (a small lamp converges). The render and --radiance; not with --adaptive, nor with --env-sampling.\n"
              << "\t   --texture\tMode X, the sphere scenes (three, weekend, stress100k): FILE.pfm[,repeat|clamp]: an image texture from a colour PFM, up to\n"
              << "\t\t\t8192 on a side (default: repeat). Each use takes the next slot, from 0. Not with --env-sampling or --light-sampling.\n"
              << "\t   --bind-sphere\tWith --texture: INDEX=SLOT or all=SLOT: the sphere of that index (or every sphere) takes the texture of that slot as\n"
              << "\t\t\tits albedo map (glass ignores it). May be given several times; later uses override earlier ones.\n"
              << "\t   --display\tMode X: CURVE[,TRANSFER[,EXPOSURE]]: the image written is the linear frame (with a single-frame --denoise, the\n"
              << "\t\t\tdenoised one) through a display transform: CURVE clamp | reinhard | filmic, TRANSFER linear | gamma2 | srgb (default: srgb),\n"
              << "\t\t\tEXPOSURE a positive gain, or auto: from the frame's trimmed log-average luminance (default: 1).\n"
              << "\t   --display-frames\tWith --display and a sequence (--frames or --lens-frames): also write PREFIX.<k>.ppm (.png under -f png) for every\n"
              << "\t\t\tframe k: the display transform of that frame (with --denoise PREFIX, of its temporally denoised frame); an auto exposure\n"
              << "\t\t\tfollows the sequence instead of jumping from frame to frame (rt3_display_sequence).\n"
              << "\t   --adapt\tWith --display ...,auto: BRIGHTER,DARKER: the share of the way the exposure moves per frame towards a brighter and\n"
              << "\t\t\ta darker target, in 1/1024, each 1 .. 1024 (default: 256,64).\n"
              << "\t   --bloom\tWith --display: LEVELS[,THRESHOLD[,INTENSITY]]: add INTENSITY times a bloom pyramid of LEVELS levels (1 .. 8) of what\n"
              << "\t\t\texceeds THRESHOLD after the exposure, before the tone curve (default: threshold 1, intensity 0.25).\n"
              << "\t   --lens\tMode X: equirect | fisheye | ortho | cube: render the frame of that lens model (rt3_render_lens) at the scene's camera\n"
              << "\t\t\tposition, looking where the camera looks, instead of the camera's; cube needs -H equal to 6 times -W (the layout --env reads).\n"
              << "\t\t\t--hdr, --aov, --denoise and --display act on the lens frame. Not with --adaptive, --frames (a sequence: --lens-frames) or --gpus above 1.\n"
              << "\t   --lens-frames\tWith --lens: render a sequence of N lens frames, frame k with seed + k; --orbit turns the lens's origin as it turns the\n"
              << "\t\t\tcamera's look-from point, --slide and --refit move the spheres, and --denoise PREFIX writes PREFIX.<k>.pfm for every frame,\n"
              << "\t\t\tdenoised temporally through the lens (rt3_denoise_temporal_optic). The image written is the last frame.\n"
              << "\t   --lens-fov\tWith --lens fisheye: the field of view across the shorter image side, in degrees, above 0 up to 360 (default: 180).\n"
              << "\t   --lens-extent\tWith --lens ortho: W,H: the width and height of the window the parallel rays start from (default: 2,2).\n"
              << "\n\t-h,--help\tShows this help menu, then exits.\n\n";
}

// Parses an unsigned option value; prints the reference's message and returns false on failure.
bool parse_u32(const std::string& text, const char* what_lower, const char* what_cap, uint32_t* out) {
    try {
        size_t used = 0;
        const unsigned long v = std::stoul(text, &used);
        if (v > std::numeric_limits<uint32_t>::max()) { std::cerr << what_cap << " too large '" + text + "'"; return false; }
        *out = (uint32_t)v;
        return true;
    } catch (std::invalid_argument&) {
        std::cerr << "Invalid " << what_lower << " '" + text + "'";
    } catch (std::out_of_range&) {
        std::cerr << what_cap << " too large '" + text + "'";
    }
    return false;
}

// "a,b,c" -> the numbers, at most cap of them: how many there are, -1 if a field is not a finite number or there are more than cap.
int parse_numbers(const std::string& text, double* out, int cap) {
    int n = 0;
    size_t at = 0;
    for (;;) {
        const size_t comma = text.find(',', at);
        const std::string field = text.substr(at, comma == std::string::npos ? comma : comma - at);
        char* end = nullptr;
        const double v = std::strtod(field.c_str(), &end);
        if (n == cap || field.empty() || end == field.c_str() || *end != '\0' || !std::isfinite(v)) return -1;
        out[n++] = v;
        if (comma == std::string::npos) return n;
        at = comma + 1;
    }
}

// 1 = go on, 0 = help was shown, -1 = usage error (the three return values of the reference's parse_cli)
int parse_cli(Options& opt, int argc, const char** argv) {
    bool have_path = false;
    for (int i = 1; i < argc; i++) {
        const std::string arg = argv[i];
        if (arg.empty() || arg[0] != '-') {
            if (!have_path) { opt.output_path = arg; have_path = true; }
            continue;                                               // extra positionals are ignored (Main.cpp:218-228)
        }
        // split "-Wvalue" / "--key=value" / "--key value"
        std::string key = arg, value;
        if (arg.size() > 1 && arg[1] != '-') { key = arg.substr(0, 2); value = arg.substr(2); }
        else if (arg.find('=') != std::string::npos) { key = arg.substr(0, arg.find('=')); value = arg.substr(arg.find('=') + 1); }

        if (key == "-h" || key == "--help") { print_usage(argv[0]); return 0; }
        if (key == "--gpu-prerender") { opt.gpu_prerender = true; continue; }
        if (key == "--dump-scene") { opt.dump_scene = true; continue; }
        if (key == "--refit") { opt.refit = true; continue; }
        if (key == "--env-sampling") { opt.env_sampling = true; continue; }
        if (key == "--light-sampling") { opt.light_sampling = true; continue; }
        const bool known = key == "-f" || key == "--format" || key == "-W" || key == "--width" || key == "-H" || key == "--height" ||
                           key == "--scene" || key == "--spp" || key == "--depth" || key == "--seed" || key == "--gpus" ||
                           key == "--aov" || key == "--hdr" || key == "--denoise" || key == "--frames" || key == "--orbit" ||
                           key == "--slide" || key == "--adaptive" || key == "--counts" || key == "--regroup" ||
                           key == "--rays" || key == "--radiance" || key == "--env" || key == "--display" || key == "--lens" || key == "--lens-fov" ||
                           key == "--lens-extent" || key == "--lens-frames" || key == "--display-frames" || key == "--adapt" || key == "--bloom" ||
                           key == "--texture" || key == "--bind-sphere" || key == "--aov-specular";
        if (!known) {
            std::cerr << "Unknown option '" << argv[i] << "'\n\n" << "Run '" << argv[0] << " -h' to see a list of valid options.\n\n";
            return -1;
        }
        if (value.empty()) {
            // (a --slide value may start with a minus sign: "-0.1,0,0")
            const bool negative_number = key == "--slide" && i < argc - 1 && argv[i + 1][0] == '-' &&
                                         (std::isdigit((unsigned char)argv[i + 1][1]) || argv[i + 1][1] == '.');
            if (i == argc - 1 || (argv[i + 1][0] == '-' && !negative_number)) { std::cerr << key << " has no value." << std::endl; return -1; }
            value = argv[++i];
        }
        if (key == "-f" || key == "--format") {
            if (value == "png") opt.png = true;
            else if (value == "ppm") opt.png = false;
            else { std::cerr << "Unknown output format '" << value << "'" << std::endl; return -1; }
        } else if (key == "-W" || key == "--width") { if (!parse_u32(value, "width", "Width", &opt.width)) return -1; }
        else if (key == "-H" || key == "--height") { if (!parse_u32(value, "height", "Height", &opt.height)) return -1; }
        else if (key == "--spp") { if (!parse_u32(value, "spp", "Spp", &opt.spp)) return -1; }
        else if (key == "--depth") { if (!parse_u32(value, "depth", "Depth", &opt.depth)) return -1; }
        else if (key == "--seed") { if (!parse_u32(value, "seed", "Seed", &opt.seed)) return -1; }
        else if (key == "--gpus") { if (!parse_u32(value, "gpus", "Gpus", &opt.gpus)) return -1; }
        else if (key == "--aov") opt.aov_prefix = value;
        else if (key == "--aov-specular") {                          // BOUNCES[,MAX_FUZZ]
            const size_t comma = value.find(',');
            if (!parse_u32(value.substr(0, comma), "aov-specular", "Aov-specular", &opt.chain.max_bounces)) return -1;
            if (comma != std::string::npos) {
                const std::string fz = value.substr(comma + 1);
                char* end = nullptr;
                const double f = std::strtod(fz.c_str(), &end);
                if (end == fz.c_str() || *end != '\0' || !(f >= 0.0) || !std::isfinite((float)f)) {
                    std::cerr << "Invalid aov-specular fuzz '" << fz << "'" << std::endl;
                    return -1;
                }
                opt.chain.max_fuzz = (float)f;
            }
            if (opt.chain.max_bounces > 16u) { std::cerr << "--aov-specular follows at most 16 bounces." << std::endl; return -1; }
            opt.aov_specular = true;
        }
        else if (key == "--hdr") opt.hdr_path = value;
        else if (key == "--denoise") opt.denoise_path = value;
        else if (key == "--frames") { if (!parse_u32(value, "frames", "Frames", &opt.frames)) return -1; }
        else if (key == "--orbit") {
            char* end = nullptr;
            const double deg = std::strtod(value.c_str(), &end);
            if (end == value.c_str() || *end != '\0' || !std::isfinite(deg) || !std::isfinite((float)deg)) {
                std::cerr << "Invalid orbit '" << value << "'" << std::endl;
                return -1;
            }
            opt.orbit = (float)deg; opt.have_orbit = true;
        }
        else if (key == "--slide") {                                 // three finite numbers, comma-separated
            const char* at = value.c_str();
            bool ok = true;
            for (int c = 0; c < 3 && ok; c++) {
                char* end = nullptr;
                const double v = std::strtod(at, &end);
                ok = end != at && std::isfinite(v) && std::isfinite((float)v) && *end == (c < 2 ? ',' : '\0');
                opt.slide[c] = (float)v;
                at = end + 1;
            }
            if (!ok) { std::cerr << "Invalid slide '" << value << "'" << std::endl; return -1; }
            opt.have_slide = true;
        }
        else if (key == "--adaptive") {                              // T[,MIN[,STEP]]: a finite T > 0, MIN >= 2, STEP >= 1
            char* end = nullptr;
            const double t = std::strtod(value.c_str(), &end);
            bool ok = end != value.c_str() && std::isfinite(t) && (float)t > 0.0f && std::isfinite((float)t) && (*end == ',' || *end == '\0');
            uint32_t* const fields[2] = { &opt.adaptive_min, &opt.adaptive_step };
            for (int c = 0; c < 2 && ok && *end == ','; c++) {
                const char* at = end + 1;
                ok = std::isdigit((unsigned char)*at) != 0;
                const unsigned long long v = ok ? std::strtoull(at, &end, 10) : 0ull;
                ok = ok && v <= std::numeric_limits<uint32_t>::max() && v >= (c == 0 ? 2ull : 1ull) && (*end == '\0' || (c == 0 && *end == ','));
                *fields[c] = (uint32_t)v;
            }
            if (!ok || *end != '\0') { std::cerr << "Invalid adaptive '" << value << "'" << std::endl; return -1; }
            opt.adaptive = true; opt.adaptive_threshold = (float)t;
        }
        else if (key == "--counts") opt.counts_path = value;
        else if (key == "--rays") opt.rays_path = value;
        else if (key == "--radiance") opt.radiance_path = value;
        else if (key == "--env") opt.env_path = value;
        else if (key == "--texture") {                               // FILE.pfm[,repeat|clamp]
            Options::Texture t{ value, RT3_TEX_REPEAT };
            const size_t comma = value.rfind(',');
            if (comma != std::string::npos) {
                const std::string mode = value.substr(comma + 1);
                if (mode == "repeat" || mode == "clamp") { t.path = value.substr(0, comma); t.wrap = mode == "clamp" ? RT3_TEX_CLAMP : RT3_TEX_REPEAT; }
                else { std::cerr << "Invalid texture wrap '" << mode << "'" << std::endl; return -1; }
            }
            if (t.path.empty() || opt.textures.size() == RT3_TEX_MAX_TEXTURES) { std::cerr << "Invalid texture '" << value << "'" << std::endl; return -1; }
            opt.textures.push_back(t);
        }
        else if (key == "--bind-sphere") {                           // INDEX=SLOT | all=SLOT
            const size_t eq = value.find('=');
            const std::string who = value.substr(0, eq), slot = eq == std::string::npos ? "" : value.substr(eq + 1);
            Options::SphereBind b{ who == "all", 0u, 0u };
            char* end = nullptr;
            bool ok = !slot.empty() && std::isdigit((unsigned char)slot[0]);
            const unsigned long long s = ok ? std::strtoull(slot.c_str(), &end, 10) : 0ull;
            ok = ok && *end == '\0' && s < RT3_TEX_MAX_TEXTURES;
            if (ok && !b.all) {
                ok = !who.empty() && std::isdigit((unsigned char)who[0]);
                const unsigned long long i = ok ? std::strtoull(who.c_str(), &end, 10) : 0ull;
                ok = ok && *end == '\0' && i <= std::numeric_limits<uint32_t>::max();
                b.index = (uint32_t)i;
            }
            if (!ok) { std::cerr << "Invalid bind-sphere '" << value << "'" << std::endl; return -1; }
            b.slot = (uint32_t)s;
            opt.sphere_binds.push_back(b);
        }
        else if (key == "--display") {                               // CURVE[,TRANSFER[,EXPOSURE]]
            const size_t c1 = value.find(','), c2 = c1 == std::string::npos ? c1 : value.find(',', c1 + 1);
            const std::string curve = value.substr(0, c1);
            const std::string transfer = c1 == std::string::npos ? "srgb" : value.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1);
            const std::string exposure = c2 == std::string::npos ? "1" : value.substr(c2 + 1);
            rt3_display_params& dp = opt.display_params;
            if (curve == "clamp") dp.curve = RT3_DISPLAY_CLAMP;
            else if (curve == "reinhard") dp.curve = RT3_DISPLAY_REINHARD;
            else if (curve == "filmic") dp.curve = RT3_DISPLAY_FILMIC;
            else { std::cerr << "Unknown display curve '" << curve << "'" << std::endl; return -1; }
            if (transfer == "linear") dp.transfer = RT3_DISPLAY_LINEAR;
            else if (transfer == "gamma2") dp.transfer = RT3_DISPLAY_GAMMA2;
            else if (transfer == "srgb") dp.transfer = RT3_DISPLAY_SRGB;
            else { std::cerr << "Unknown display transfer '" << transfer << "'" << std::endl; return -1; }
            if (exposure == "auto") { dp.flags = RT3_DISPLAY_AUTO_EXPOSURE; dp.exposure = 1.0f; }
            else {
                char* end = nullptr;
                const double e = std::strtod(exposure.c_str(), &end);
                if (end == exposure.c_str() || *end != '\0' || !std::isfinite(e) || !((float)e > 0.0f) || !std::isfinite((float)e)) {
                    std::cerr << "Invalid display exposure '" << exposure << "'" << std::endl;
                    return -1;
                }
                dp.flags = 0u; dp.exposure = (float)e;
            }
            opt.display = true;
        }
        else if (key == "--display-frames") opt.display_frames = value;
        else if (key == "--adapt") {                                 // BRIGHTER,DARKER in 1/1024
            double v[3];
            if (parse_numbers(value, v, 3) != 2 || !(v[0] >= 1.0 && v[0] <= 1024.0 && v[1] >= 1.0 && v[1] <= 1024.0) || v[0] != std::floor(v[0]) ||
                v[1] != std::floor(v[1])) {
                std::cerr << "Invalid adapt '" << value << "' (BRIGHTER,DARKER: two whole numbers 1 .. 1024)" << std::endl;
                return -1;
            }
            opt.adapt[0] = (uint32_t)v[0]; opt.adapt[1] = (uint32_t)v[1]; opt.have_adapt = true;
        }
        else if (key == "--bloom") {                                 // LEVELS[,THRESHOLD[,INTENSITY]]
            double v[4] = { 0.0, 1.0, 0.25, 0.0 };
            const int n = parse_numbers(value, v, 4);
            if (n < 1 || n > 3 || !(v[0] >= 1.0 && v[0] <= 8.0) || v[0] != std::floor(v[0]) || !(v[1] >= 0.0) || !std::isfinite((float)v[1]) ||
                !(v[2] >= 0.0) || !std::isfinite((float)v[2])) {
                std::cerr << "Invalid bloom '" << value << "' (LEVELS[,THRESHOLD[,INTENSITY]]: 1 .. 8 levels, a threshold and an intensity of at least 0)" << std::endl;
                return -1;
            }
            opt.bloom_levels = (uint32_t)v[0]; opt.bloom_threshold = (float)v[1]; opt.bloom_intensity = (float)v[2]; opt.have_bloom = true;
        }
        else if (key == "--lens") {
            if (value == "equirect") opt.lens = RT3_LENS_EQUIRECT;
            else if (value == "fisheye") opt.lens = RT3_LENS_FISHEYE;
            else if (value == "ortho") opt.lens = RT3_LENS_ORTHO;
            else if (value == "cube") opt.lens = RT3_LENS_CUBE;
            else { std::cerr << "Unknown lens '" << value << "'" << std::endl; return -1; }
        }
        else if (key == "--lens-frames") { if (!parse_u32(value, "lens-frames", "Lens-frames", &opt.lens_frames)) return -1; opt.have_lens_frames = true; }
        else if (key == "--lens-fov") {                              // degrees in (0, 360]
            char* end = nullptr;
            const double deg = std::strtod(value.c_str(), &end);
            if (end == value.c_str() || *end != '\0' || !(deg > 0.0) || !(deg <= 360.0)) { std::cerr << "Invalid lens-fov '" << value << "'" << std::endl; return -1; }
            opt.lens_fov = (float)deg; opt.have_lens_fov = true;
        }
        else if (key == "--lens-extent") {                           // W,H: two finite numbers above 0
            const char* at = value.c_str();
            bool ok = true;
            for (int c = 0; c < 2 && ok; c++) {
                char* end = nullptr;
                const double v = std::strtod(at, &end);
                ok = end != at && std::isfinite(v) && (float)v > 0.0f && std::isfinite((float)v) && *end == (c < 1 ? ',' : '\0');
                opt.lens_extent[c] = (float)v;
                at = end + 1;
            }
            if (!ok) { std::cerr << "Invalid lens-extent '" << value << "'" << std::endl; return -1; }
            opt.have_lens_extent = true;
        }
        else if (key == "--regroup") {
            if (!parse_u32(value, "regroup", "Regroup", &opt.regroup)) return -1;
            if (opt.regroup == 0) { std::cerr << "--regroup must be at least 1." << std::endl; return -1; }
            opt.have_regroup = true;
        }
        else opt.scene = value;
    }
    if (opt.output_path.empty() && !opt.dump_scene) { std::cerr << "No output path given." << std::endl; return -1; }
    // the builtin scene and .scene files render in Mode R unless --spp is given; the analytic scenes always run Mode X
    const bool mode_r = opt.spp == 0 && (opt.scene == "builtin" || (opt.scene.size() > 6 && opt.scene.compare(opt.scene.size() - 6, 6, ".scene") == 0));
    if (mode_r && (!opt.aov_prefix.empty() || !opt.hdr_path.empty())) {
        std::cerr << "--aov and --hdr need the path tracer (Mode X): pass --spp." << std::endl;
        return -1;
    }
    if (opt.aov_specular && mode_r) { std::cerr << "--aov-specular needs the path tracer (Mode X): pass --spp." << std::endl; return -1; }
    if (opt.aov_specular && (opt.frames > 1 || opt.lens_frames > 1)) {
        std::cerr << "--aov-specular is not available with --frames or --lens-frames: the temporal denoisers rebuild the first-hit point from depth." << std::endl;
        return -1;
    }
    if (mode_r && !opt.denoise_path.empty()) {
        std::cerr << "--denoise needs the path tracer (Mode X): pass --spp." << std::endl;
        return -1;
    }
    if (opt.rays_path.empty() != opt.radiance_path.empty()) {
        std::cerr << "--rays and --radiance go together: the rays to trace and where their radiance is written." << std::endl;
        return -1;
    }
    if (mode_r && !opt.rays_path.empty()) {
        std::cerr << "--rays and --radiance need the path tracer (Mode X): pass --spp." << std::endl;
        return -1;
    }
    if (mode_r && !opt.env_path.empty()) {
        std::cerr << "--env needs the path tracer (Mode X): pass --spp." << std::endl;
        return -1;
    }
    if (opt.env_sampling && opt.env_path.empty()) {
        std::cerr << "--env-sampling needs --env." << std::endl;
        return -1;
    }
    if (opt.env_sampling && opt.adaptive) {
        std::cerr << "--env-sampling is not available with --adaptive." << std::endl;
        return -1;
    }
    if (!opt.textures.empty() || !opt.sphere_binds.empty()) {
        const char* why = mode_r ? "--texture and --bind-sphere need the path tracer (Mode X): pass --spp."
                        : !(opt.scene == "three" || opt.scene == "weekend" || opt.scene == "stress100k") ? "--texture and --bind-sphere need a sphere scene (three, weekend, stress100k)."
                        : opt.env_sampling || opt.light_sampling ? "--texture is not available with --env-sampling or --light-sampling."
                        : nullptr;
        for (const Options::SphereBind& b : opt.sphere_binds)
            if (!why && b.slot >= opt.textures.size()) why = "--bind-sphere names a slot that no --texture fills.";
        if (why) { std::cerr << why << std::endl; return -1; }
    }
    if (mode_r && opt.light_sampling) {
        std::cerr << "--light-sampling needs the path tracer (Mode X): pass --spp." << std::endl;
        return -1;
    }
    if (opt.light_sampling && opt.env_sampling) {
        std::cerr << "--light-sampling is not available with --env-sampling." << std::endl;
        return -1;
    }
    if (opt.light_sampling && opt.adaptive) {
        std::cerr << "--light-sampling is not available with --adaptive." << std::endl;
        return -1;
    }
    if (mode_r && opt.display) {
        std::cerr << "--display needs the path tracer (Mode X): pass --spp." << std::endl;
        return -1;
    }
    if (!opt.display_frames.empty() && !opt.display) {
        std::cerr << "--display-frames needs --display: it is the transform every frame goes through." << std::endl;
        return -1;
    }
    if (!opt.display_frames.empty() && opt.frames < 2 && opt.lens_frames < 2) {
        std::cerr << "--display-frames needs a sequence: pass --frames N (with --lens: --lens-frames N) with N of at least 2." << std::endl;
        return -1;
    }
    if (opt.have_adapt && !(opt.display && (opt.display_params.flags & RT3_DISPLAY_AUTO_EXPOSURE))) {
        std::cerr << "--adapt needs --display with the auto exposure: a given exposure does not move." << std::endl;
        return -1;
    }
    if (opt.have_bloom && !opt.display) {
        std::cerr << "--bloom needs --display: it is added before the tone curve." << std::endl;
        return -1;
    }
    if (mode_r && opt.adaptive) {
        std::cerr << "--adaptive needs the path tracer (Mode X): pass --spp, the budget." << std::endl;
        return -1;
    }
    if (!opt.counts_path.empty() && !opt.adaptive) {
        std::cerr << "--counts needs --adaptive: a uniform render gives every pixel --spp samples." << std::endl;
        return -1;
    }
    if (opt.frames == 0) { std::cerr << "--frames must be at least 1." << std::endl; return -1; }
    if ((opt.have_lens_fov || opt.have_lens_extent) && opt.lens == 0) {
        std::cerr << "--lens-fov and --lens-extent need --lens." << std::endl;
        return -1;
    }
    if (opt.have_lens_frames && opt.lens == 0) { std::cerr << "--lens-frames needs --lens: a camera sequence is --frames." << std::endl; return -1; }
    if (opt.have_lens_frames && opt.lens_frames == 0) { std::cerr << "--lens-frames must be at least 1." << std::endl; return -1; }
    if (opt.lens != 0) {
        if (opt.spp == 0) { std::cerr << "--lens needs the path tracer (Mode X): pass --spp." << std::endl; return -1; }
        if (opt.adaptive) { std::cerr << "--lens is not available with --adaptive." << std::endl; return -1; }
        if (opt.frames > 1) { std::cerr << "--lens renders one frame: it is not available with --frames." << std::endl; return -1; }
        if (opt.gpus > 1) { std::cerr << "--lens renders on one device: it is not available with --gpus above 1." << std::endl; return -1; }
        if (!opt.rays_path.empty()) { std::cerr << "--lens is not available with --rays and --radiance." << std::endl; return -1; }
        if (opt.lens == RT3_LENS_CUBE && (uint64_t)opt.height != 6ull * opt.width) {
            std::cerr << "--lens cube needs a frame of six stacked faces: -H must be 6 times -W." << std::endl;
            return -1;
        }
    }
    if (mode_r && opt.frames > 1) {
        std::cerr << "--frames needs the path tracer (Mode X): pass --spp." << std::endl;
        return -1;
    }
    if (opt.have_orbit && opt.scene != "weekend" && opt.scene != "stress100k") {
        std::cerr << "--orbit needs a look-at camera (--scene weekend or stress100k)." << std::endl;
        return -1;
    }
    if (opt.have_slide && opt.scene != "three" && opt.scene != "weekend" && opt.scene != "stress100k") {
        std::cerr << "--slide needs a sphere scene (--scene three, weekend or stress100k)." << std::endl;
        return -1;
    }
    if (opt.have_slide && opt.frames < 2 && opt.lens_frames < 2) {
        std::cerr << "--slide needs a sequence: pass --frames N with N of at least 2." << std::endl;
        return -1;
    }
    if (opt.refit && !opt.have_slide) {
        std::cerr << "--refit needs --slide: it is how the moved spheres reach the device." << std::endl;
        return -1;
    }
    if (opt.have_regroup && !opt.refit) {
        std::cerr << "--regroup needs --refit: a full upload sorts the groups itself." << std::endl;
        return -1;
    }
    return 1;
}

// The spheres of the scene on the renderer (--slide moves them from frame to frame).
std::vector<float> scene_cr;
std::vector<rt3_material> scene_mats;

// --env: a colour PFM ("PF", little-endian: a negative scale), N wide and 6N high -> the texels rt3_set_environment takes.  A PFM stores its rows
// bottom to top; with that undone, rows [f N, (f + 1) N) from the top are face f, its row 0 first.
std::vector<float> read_env_pfm(const std::string& path, uint32_t& n_face) {
    std::ifstream in(path, std::ios::binary);
    if (!in) throw Fatal("Could not open '" + path + "'");
    std::string magic;
    long long w = 0, h = 0;
    double scale = 0.0;
    in >> magic >> w >> h >> scale;
    if (!in || in.get() == EOF) throw Fatal("'" + path + "' is not a PFM file");
    if (magic != "PF" || !(scale < 0.0)) throw Fatal("'" + path + "' must be a little-endian colour PFM (PF, negative scale)");
    if (w < 1 || w > (long long)RT3_ENV_MAX_FACE || h != 6 * w)
        throw Fatal("'" + path + "' is " + std::to_string(w) + " x " + std::to_string(h) + ": an environment map is N wide and 6N high, N up to " +
                    std::to_string(RT3_ENV_MAX_FACE));
    std::vector<float> rgb((size_t)3 * w * h);
    if (!in.read(reinterpret_cast<char*>(rgb.data()), (std::streamsize)(rgb.size() * sizeof(float)))) throw Fatal("'" + path + "' ends before its pixels do");
    std::vector<float> rgba((size_t)4 * w * h, 0.0f);
    for (long long y = 0; y < h; y++)                                // y: row from the top = texel row of the stacked faces
        for (long long x = 0; x < w; x++)
            for (int c = 0; c < 3; c++) rgba[4 * (size_t)(y * w + x) + c] = rgb[3 * (size_t)((h - 1 - y) * w + x) + c];
    n_face = (uint32_t)w;
    return rgba;
}

// --texture: a colour PFM, W wide and H high -> the texels rt3_set_texture takes, row 0 on top (a PFM stores its rows bottom to top).
std::vector<float> read_texture_pfm(const std::string& path, uint32_t& w_out, uint32_t& h_out) {
    std::ifstream in(path, std::ios::binary);
    if (!in) throw Fatal("Could not open '" + path + "'");
    std::string magic;
    long long w = 0, h = 0;
    double scale = 0.0;
    in >> magic >> w >> h >> scale;
    if (!in || in.get() == EOF) throw Fatal("'" + path + "' is not a PFM file");
    if (magic != "PF" || !(scale < 0.0)) throw Fatal("'" + path + "' must be a little-endian colour PFM (PF, negative scale)");
    if (w < 1 || h < 1 || w > (long long)RT3_TEX_MAX_SIDE || h > (long long)RT3_TEX_MAX_SIDE || w * h > (1ll << 26))
        throw Fatal("'" + path + "' is " + std::to_string(w) + " x " + std::to_string(h) + ": a texture is up to " + std::to_string(RT3_TEX_MAX_SIDE) +
                    " on a side and holds up to 2^26 texels");
    std::vector<float> rgb((size_t)3 * w * h);
    if (!in.read(reinterpret_cast<char*>(rgb.data()), (std::streamsize)(rgb.size() * sizeof(float)))) throw Fatal("'" + path + "' ends before its pixels do");
    std::vector<float> rgba((size_t)4 * w * h, 0.0f);
    for (long long y = 0; y < h; y++)                                // y: row from the top
        for (long long x = 0; x < w; x++)
            for (int c = 0; c < 3; c++) rgba[4 * (size_t)(y * w + x) + c] = rgb[3 * (size_t)((h - 1 - y) * w + x) + c];
    w_out = (uint32_t)w; h_out = (uint32_t)h;
    return rgba;
}

template <class Fn>
void sphere_scene(HipRenderer& r, Fn generate) {
    const uint32_t n = generate(nullptr, nullptr, 0);
    std::vector<float>& cr = scene_cr;
    std::vector<rt3_material>& mats = scene_mats;
    cr.assign(4 * (size_t)n, 0.0f);
    mats.assign(n, rt3_material{});
    generate(cr.data(), mats.data(), n);
    r.prerender(Tools::Array<ECS::RenderEntity*>());
    r.set_spheres(cr, mats);
}

}  // namespace

int main(int argc, const char** argv) {
    Options opt;
    const int parsed = parse_cli(opt, argc, argv);
    if (parsed <= 0) return parsed;

    if (opt.dump_scene) {                                            // parse a .scene file and print its entities (no GPU needed)
        try {
            Tools::Array<ECS::RenderEntity*> entities = SceneParser::parse_file(opt.scene);
            for (size_t i = 0; i < entities.size(); i++) {
                const ECS::RenderEntity* e = entities[i];
                std::cout << ECS::entity_type_names[e->type] << " faces=" << e->pre_render_faces << " vertices=" << e->pre_render_vertices;
                if (e->type == ECS::et_triangle) { const auto* t = static_cast<const ECS::Triangle*>(e); for (int k = 0; k < 3; k++) std::cout << " p" << k + 1 << "=(" << t->points[k].x << "," << t->points[k].y << "," << t->points[k].z << ")"; std::cout << " color=(" << t->color.x << "," << t->color.y << "," << t->color.z << ")"; }
                if (e->type == ECS::et_sphere || e->type == ECS::et_analytic_sphere) { const auto* s = static_cast<const ECS::Sphere*>(e); std::cout << " center=(" << s->center.x << "," << s->center.y << "," << s->center.z << ") radius=" << s->radius << " grid=" << s->n_meridians << "x" << s->n_parallels << " color=(" << s->color.x << "," << s->color.y << "," << s->color.z << ")"; }
                if (e->type == ECS::et_object) { const auto* o = static_cast<const ECS::Object*>(e); std::cout << " center=(" << o->center.x << "," << o->center.y << "," << o->center.z << ") scale=" << o->scale << " color=(" << o->color.x << "," << o->color.y << "," << o->color.z << ")"; }
                if (e->has_material) std::cout << " material=" << e->material.kind << " param=" << e->material.param;
                std::cout << "\n";
                delete e;
            }
            return 0;
        } catch (Fatal& e) { std::cerr << "fatal: " << e.what() << std::endl; return -1; }
    }

    try {
        std::vector<int> devices;
        for (uint32_t i = 0; i < (opt.gpus ? opt.gpus : 1); i++) devices.push_back((int)i);
        // RT3_DEVICE_LIST="0,0,0" (testing aid): the device behind each of the --gpus shards, so that the multi-device path —
        // device tiles, device-to-device gather into shard 0's frame — can be exercised on a box with a single GPU
        if (const char* list = std::getenv("RT3_DEVICE_LIST")) {
            devices.clear();
            std::stringstream ss(list);
            std::string item;
            while (std::getline(ss, item, ',')) if (!item.empty()) devices.push_back(std::atoi(item.c_str()));
            if (devices.empty()) devices.push_back(0);
        }
        HipRenderer renderer(devices);
        renderer.set_gpu_prerender(opt.gpu_prerender);
        Camera cam;
        PathOptions path;
        path.spp = opt.spp; path.max_depth = opt.depth ? opt.depth : 1; path.seed = opt.seed;
        const float aspect = (float)opt.width / (float)opt.height;
        struct { bool on = false; glm::vec3 from, at, vup; float vfov = 0.0f, focus = 0.0f; } la;     // the look-at scenes' camera

        if (opt.scene == "builtin") {                               // Main.cpp:272, :280-283
            cam.update(opt.width, opt.height, 2.0f, aspect * 2.0f, 2.0f);
            Tools::Array<ECS::RenderEntity*> entities({
                ECS::create_object("bin/objects/teddy.obj", { 0.0f, 0.0f, -3.0f }, 1.0f / 17.0f, { 1.0f, 0.0f, 0.0f }),
                ECS::create_sphere({ -2.0f, 0.0f, -5.0f }, 1.0f, 8, 8, { 0.0f, 0.0f, 1.0f }) });
            renderer.prerender(entities);
            for (size_t i = 0; i < entities.size(); i++) delete entities[i];
        } else if (opt.scene == "three") {
            cam.update(opt.width, opt.height, 1.0f, aspect * 2.0f, 2.0f);
            sphere_scene(renderer, [](float* c, rt3_material* m, uint32_t cap) { return rt3_scene_three_spheres(c, m, cap); });
            path.flags = RT3_FLAG_GAMMA2;
        } else if (opt.scene == "weekend") {
            la.on = true; la.from = { 13.0f, 2.0f, 3.0f }; la.at = { 0.0f, 0.0f, 0.0f }; la.vup = { 0.0f, 1.0f, 0.0f }; la.vfov = 20.0f; la.focus = 10.0f;
            sphere_scene(renderer, [](float* c, rt3_material* m, uint32_t cap) { return rt3_scene_weekend(42, c, m, cap); });
            path.flags = RT3_FLAG_GAMMA2; path.lens_radius = 0.05f;
        } else if (opt.scene == "stress100k") {
            la.on = true; la.from = { 0.0f, 8.0f, 12.0f }; la.at = { 0.0f, 6.0f, -50.0f }; la.vup = { 0.0f, 1.0f, 0.0f }; la.vfov = 45.0f; la.focus = 1.0f;
            sphere_scene(renderer, [](float* c, rt3_material* m, uint32_t cap) { return rt3_scene_stress(100000, 43, c, m, cap); });
            path.flags = RT3_FLAG_GAMMA2;
        } else if (opt.scene == "cornell") {
            cam.update(opt.width, opt.height, 2.0f, aspect * 2.0f, 2.0f);
            const uint32_t n = rt3_scene_cornell(64, nullptr, nullptr, nullptr, 0);
            std::vector<rt3_gface> faces(n); std::vector<float> verts(12 * (size_t)n); std::vector<rt3_material> mats(n);
            rt3_scene_cornell(64, faces.data(), verts.data(), mats.data(), n);
            renderer.prerender(Tools::Array<ECS::RenderEntity*>());
            renderer.set_mesh(faces, verts, mats);
            path.flags = RT3_FLAG_GAMMA2 | RT3_FLAG_BLACK_BACKGROUND;
        } else if (opt.scene.size() > 6 && opt.scene.compare(opt.scene.size() - 6, 6, ".scene") == 0) {   // a SceneLang file
            cam.update(opt.width, opt.height, 2.0f, aspect * 2.0f, 2.0f);
            Tools::Array<ECS::RenderEntity*> entities = SceneParser::parse_file(opt.scene);
            renderer.prerender(entities);
            for (size_t i = 0; i < entities.size(); i++) delete entities[i];
            path.flags = opt.spp ? RT3_FLAG_GAMMA2 : 0;
        } else {
            std::cerr << "Unknown scene '" << opt.scene << "'" << std::endl;
            return -1;
        }
        const bool from_file = opt.scene.size() > 6 && opt.scene.compare(opt.scene.size() - 6, 6, ".scene") == 0;
        if (opt.scene != "builtin" && !from_file && path.spp == 0) path.spp = 16;   // the analytic scenes only exist in Mode X
        if (!opt.env_path.empty()) {
            uint32_t n_face = 0;
            const std::vector<float> rgba = read_env_pfm(opt.env_path, n_face);
            renderer.set_environment(rgba, n_face);
            if (opt.env_sampling) path.flags |= RT3_FLAG_ENV_SAMPLING;
        }
        if (opt.light_sampling) path.flags |= RT3_FLAG_LIGHT_SAMPLING;
        // --texture / --bind-sphere: the slots once, the spheres' binding now and again after every full upload of the spheres (it goes with them)
        std::vector<uint32_t> sphere_slots;
        for (size_t k = 0; k < opt.textures.size(); k++) {
            uint32_t tw = 0, th = 0;
            const std::vector<float> rgba = read_texture_pfm(opt.textures[k].path, tw, th);
            renderer.set_texture((uint32_t)k, rgba, tw, th, opt.textures[k].wrap);
        }
        if (!opt.sphere_binds.empty()) {
            sphere_slots.assign(scene_mats.size(), RT3_TEX_NONE);
            for (const Options::SphereBind& b : opt.sphere_binds) {
                if (b.all) std::fill(sphere_slots.begin(), sphere_slots.end(), b.slot);
                else if (b.index < sphere_slots.size()) sphere_slots[b.index] = b.slot;
                else throw Fatal("--bind-sphere: the scene has no sphere " + std::to_string(b.index));
            }
            renderer.bind_sphere_textures(sphere_slots);
        }
        const uint32_t seed0 = path.seed;
        const rt3_temporal_params tp{ { 5, 128, 4.0f, 1.0f }, 0.2f, 0.2f, 2.0f, 0.9f };       // the defaults of DESIGN.md 4.11 and 4.12
        std::vector<float> shown_cr = scene_cr, prev_cr;             // --slide: the spheres of this frame and of the one before
        // --slide, frame k > 0: every sphere of odd index translated by k * slide, uploaded or (--refit) updated in place
        const auto slide_spheres = [&](uint32_t k) {
            prev_cr = shown_cr;
            for (size_t i = 1; i < scene_mats.size(); i += 2)
                for (int c = 0; c < 3; c++) shown_cr[4 * i + c] = scene_cr[4 * i + c] + (float)k * opt.slide[c];
            if (opt.refit) {
                renderer.update_spheres(shown_cr);
                if (opt.regroup != 0 && k % opt.regroup == 0) renderer.regroup(true, false);
            }
            else {
                renderer.set_spheres(shown_cr, scene_mats);
                if (!sphere_slots.empty()) renderer.bind_sphere_textures(sphere_slots);
            }
        };
        // --orbit, frame k: the look-from point turned by k * orbit about the vertical axis through the look-at point
        const auto orbit_from = [&](uint32_t k) {
            if (k == 0) return la.from;
            const double a = (double)k * (double)opt.orbit * 3.14159265358979323846 / 180.0, c = std::cos(a), sn = std::sin(a);
            const double dx = (double)la.from.x - la.at.x, dz = (double)la.from.z - la.at.z;
            return glm::vec3(la.at.x + (c * dx + sn * dz), (double)la.from.y, la.at.z + (c * dz - sn * dx));
        };
        // --display-frames, frame k: the display transform of `frame` as one frame of the sequence (the exposure's state is carried from frame to
        // frame), written as PREFIX.k.ppm | .png.  --bloom alone: the final image goes through the same call with a state of its own.
        rt3_exposure exposure_state{};
        const auto write_display_frame = [&](uint32_t k, const std::vector<float>& frame) {
            renderer.display_sequence(cam, frame, opt.sequence_params(), exposure_state);
            const std::string name = opt.display_frames + "." + std::to_string(k) + (opt.png ? ".png" : ".ppm");
            if (opt.png) cam.get_frame().to_png(name);
            else cam.get_frame().to_ppm(name);
        };
        const auto display_image = [&](const std::vector<float>& frame) {
            rt3_exposure alone{};
            if (opt.have_bloom) renderer.display_sequence(cam, frame, opt.sequence_params(), alone);
            else renderer.display(cam, frame, opt.display_params);
        };
        if (opt.lens != 0) {                                         // the frame of another lens model, at the camera's place
            const uint32_t w = opt.width, h = opt.height;
            const float origin[3] = { 0.0f, 0.0f, 0.0f }, ahead[3] = { 0.0f, 0.0f, -1.0f }, up[3] = { 0.0f, 1.0f, 0.0f };       // the reference camera
            rt3_lens lens{};
            if (la.on) cam.look_at(w, h, la.from, la.at, la.vup, la.vfov, la.focus);      // (the camera only lends its frame buffer to the image)
            path.lens_radius = 0.0f;
            const bool temporal = opt.lens_frames > 1 && !opt.denoise_path.empty();
            LensHistory history;
            std::vector<float> linear;
            rt3_stats st{};                                          // the last frame's render (the AOV pass of a temporal frame replaces the context's)
            for (uint32_t k = 0; k < opt.lens_frames; k++) {         // (--lens-frames: frame k with seed + k, the lens's origin on --orbit's circle)
                if (opt.have_slide && k > 0) slide_spheres(k);
                if (la.on) { const glm::vec3 from = orbit_from(k); rt3_lens_look_at(&lens, opt.lens, &from.x, &la.at.x, &la.vup.x); }
                else rt3_lens_look_at(&lens, opt.lens, origin, ahead, up);
                lens.half_fov_turns = opt.lens_fov / 720.0f;
                lens.half_extent[0] = 0.5f * opt.lens_extent[0]; lens.half_extent[1] = 0.5f * opt.lens_extent[1];
                path.seed = seed0 + k;
                renderer.configure(path);
                linear = renderer.render_lens(lens, w, h);
                st = renderer.stats();
                if (temporal) {
                    const std::vector<rt3_aov> guides = renderer.lens_aov(lens, w, h);
                    std::vector<float> motion;
                    if (opt.have_slide && k > 0) motion = renderer.motion_lens(lens, w, h, guides, prev_cr, {});
                    const std::vector<float> out = renderer.denoise_temporal_lens(lens, w, h, linear, guides, tp, history, motion);
                    const std::string name = opt.denoise_path + "." + std::to_string(k) + ".pfm";
                    if (rt3_frame_to_pfm(out.data(), w, h, 3, 4, name.c_str()) != 0) throw Fatal("Could not write '" + name + "'");
                    if (!opt.display_frames.empty()) write_display_frame(k, out);
                } else if (!opt.display_frames.empty()) write_display_frame(k, linear);
            }
            std::cerr << "rendered a lens frame of " << w << "x" << h << " x " << path.spp << " spp in " << st.total_ms << " ms on device 0: " << st.ray_casts
                      << " rays, " << st.launches << " launches\n";
            const bool need_aov = !opt.aov_prefix.empty() || (!opt.denoise_path.empty() && !temporal);
            const std::vector<rt3_aov> aov = !need_aov ? std::vector<rt3_aov>()
                                             : opt.aov_specular ? renderer.lens_aov_specular(lens, w, h, opt.chain) : renderer.lens_aov(lens, w, h);
            const rt3_denoise_params dp{ 5, 128, 4.0f, 1.0f };                       // the defaults of DESIGN.md 4.11
            const std::vector<float> denoised = opt.denoise_path.empty() || temporal ? std::vector<float>() : renderer.denoise(w, h, linear, aov, dp);
            // the image: --display's transform, or the one that reproduces the ordinary Mode-X pack (no curve, the scene's gamma)
            const rt3_display_params pack{ RT3_DISPLAY_CLAMP, (path.flags & RT3_FLAG_GAMMA2) ? RT3_DISPLAY_GAMMA2 : RT3_DISPLAY_LINEAR, 0u, 102u, 51u, 1.0f, 0.18f, 4.0f };
            if (opt.display) display_image(denoised.empty() ? linear : denoised);
            else renderer.display(cam, linear, pack);
            if (opt.png) cam.get_frame().to_png(opt.output_path);
            else cam.get_frame().to_ppm(opt.output_path);
            if (!opt.hdr_path.empty() && rt3_frame_to_pfm(linear.data(), w, h, 3, 4, opt.hdr_path.c_str()) != 0) throw Fatal("Could not write '" + opt.hdr_path + "'");
            if (!opt.aov_prefix.empty()) {
                const float* base = reinterpret_cast<const float*>(aov.data());
                const struct { const char* name; size_t offset; uint32_t channels; } planes[] = { { ".albedo.pfm", 0, 3 }, { ".normal.pfm", 4, 3 }, { ".depth.pfm", 7, 1 } };
                for (const auto& pl : planes) {
                    const std::string out = opt.aov_prefix + pl.name;
                    if (rt3_frame_to_pfm(base + pl.offset, w, h, pl.channels, sizeof(rt3_aov) / sizeof(float), out.c_str()) != 0)
                        throw Fatal("Could not write '" + out + "'");
                }
            }
            if (!denoised.empty() && rt3_frame_to_pfm(denoised.data(), w, h, 3, 4, opt.denoise_path.c_str()) != 0)
                throw Fatal("Could not write '" + opt.denoise_path + "'");
            return 0;
        }
        const bool temporal = opt.frames > 1 && !opt.denoise_path.empty();
        History history;
        std::vector<uint32_t> counts;                                // --adaptive: the samples every pixel of the last frame received
        for (uint32_t k = 0; k < opt.frames; k++) {
            if (opt.have_slide && k > 0) slide_spheres(k);
            if (la.on) cam.look_at(opt.width, opt.height, orbit_from(k), la.at, la.vup, la.vfov, la.focus);
            path.seed = seed0 + k;
            renderer.configure(path);
            if (opt.adaptive) {
                const uint32_t min_spp = opt.adaptive_min ? opt.adaptive_min : (path.spp < 16u ? path.spp : 16u);
                counts = renderer.render_adaptive(cam, rt3_adaptive_params{ min_spp, opt.adaptive_step, opt.adaptive_threshold, 0.01f });
            } else renderer.render(cam);
            if (temporal) {
                std::vector<float> motion;
                if (opt.have_slide && k > 0) motion = renderer.motion(cam, prev_cr, {});
                const std::vector<float> out = renderer.denoise_temporal(cam, tp, history, motion);
                const std::string name = opt.denoise_path + "." + std::to_string(k) + ".pfm";
                if (rt3_frame_to_pfm(out.data(), cam.w(), cam.h(), 3, 4, name.c_str()) != 0) throw Fatal("Could not write '" + name + "'");
                if (!opt.display_frames.empty()) write_display_frame(k, out);
            } else if (!opt.display_frames.empty()) write_display_frame(k, renderer.hdr());
        }

        const rt3_stats st = renderer.stats();
        std::cerr << "rendered " << opt.width << "x" << opt.height << (path.spp ? " x " + std::to_string(path.spp) + " spp" : " (mode R)")
                  << " in " << st.total_ms << " ms on device 0: " << st.ray_casts << " rays, " << st.prim_tests << " ray-primitive tests\n";
        const rt3_denoise_params dp{ 5, 128, 4.0f, 1.0f };                         // the defaults of DESIGN.md 4.11
        // the single-frame denoiser: guided by the first-hit AOVs, or under --aov-specular by the chain's
        const auto denoise_frame = [&]() {
            return opt.aov_specular ? renderer.denoise(cam.w(), cam.h(), renderer.hdr(), renderer.aov_specular(cam, opt.chain), dp) : renderer.denoise(cam, dp);
        };
        std::vector<float> denoised;                                 // --display with a single-frame --denoise: the frame both outputs come from
        if (opt.display) {                                           // the image becomes the display transform of the linear frame
            if (!opt.denoise_path.empty() && !temporal) denoised = denoise_frame();
            display_image(denoised.empty() ? renderer.hdr() : denoised);
        }
        if (opt.png) cam.get_frame().to_png(opt.output_path);
        else cam.get_frame().to_ppm(opt.output_path);
        const uint32_t w = cam.w(), h = cam.h();
        if (opt.adaptive) {
            uint64_t total = 0;
            for (const uint32_t c : counts) total += c;
            std::cerr << "adaptive: " << total << " samples, " << (double)total / ((double)w * h * path.spp) << " of the uniform " << path.spp << " spp\n";
            if (!opt.counts_path.empty()) {
                const std::vector<float> as_float(counts.begin(), counts.end());
                if (rt3_frame_to_pfm(as_float.data(), w, h, 1, 1, opt.counts_path.c_str()) != 0) throw Fatal("Could not write '" + opt.counts_path + "'");
            }
        }
        if (!opt.hdr_path.empty()) {
            const std::vector<float> hdr = renderer.hdr();
            if (rt3_frame_to_pfm(hdr.data(), w, h, 3, 4, opt.hdr_path.c_str()) != 0) throw Fatal("Could not write '" + opt.hdr_path + "'");
        }
        if (!opt.aov_prefix.empty()) {
            const std::vector<rt3_aov> aov = opt.aov_specular ? renderer.aov_specular(cam, opt.chain) : renderer.aov(cam);
            const float* base = reinterpret_cast<const float*>(aov.data());          // (rt3_aov: 12 floats and words, 48 bytes)
            const struct { const char* name; size_t offset; uint32_t channels; } planes[] = { { ".albedo.pfm", 0, 3 }, { ".normal.pfm", 4, 3 }, { ".depth.pfm", 7, 1 } };
            for (const auto& pl : planes) {
                const std::string out = opt.aov_prefix + pl.name;
                if (rt3_frame_to_pfm(base + pl.offset, w, h, pl.channels, sizeof(rt3_aov) / sizeof(float), out.c_str()) != 0)
                    throw Fatal("Could not write '" + out + "'");
            }
        }
        if (!opt.denoise_path.empty() && !temporal) {
            const std::vector<float> out = denoised.empty() ? denoise_frame() : denoised;
            if (rt3_frame_to_pfm(out.data(), w, h, 3, 4, opt.denoise_path.c_str()) != 0) throw Fatal("Could not write '" + opt.denoise_path + "'");
        }
        if (!opt.rays_path.empty()) {                                // last: it replaces the render's stats, and touches nothing the outputs above read
            std::ifstream in(opt.rays_path, std::ios::binary | std::ios::ate);
            if (!in) throw Fatal("Could not open '" + opt.rays_path + "'");
            const std::streamoff bytes = in.tellg();
            if (bytes <= 0 || bytes % (std::streamoff)sizeof(rt3_ray) != 0 || bytes / (std::streamoff)sizeof(rt3_ray) > (std::streamoff)(1u << 27))
                throw Fatal("'" + opt.rays_path + "' must hold between 1 and 2^27 rt3_ray records of 32 bytes");
            std::vector<rt3_ray> rays((size_t)(bytes / (std::streamoff)sizeof(rt3_ray)));
            in.seekg(0);
            if (!in.read(reinterpret_cast<char*>(rays.data()), bytes)) throw Fatal("Could not read '" + opt.rays_path + "'");
            const std::vector<float> out = renderer.radiance(rays);
            if (rt3_frame_to_pfm(out.data(), (uint32_t)rays.size(), 1, 3, 4, opt.radiance_path.c_str()) != 0) throw Fatal("Could not write '" + opt.radiance_path + "'");
            std::cerr << "radiance: " << rays.size() << " rays x " << path.spp << " samples, " << renderer.stats().ray_casts << " ray casts\n";
        }
    } catch (Fatal& e) {
        std::cerr << "fatal: " << e.what() << std::endl;            // the reference logs and returns -1 (Main.cpp:305-308)
        return -1;
    }
    return 0;
}
