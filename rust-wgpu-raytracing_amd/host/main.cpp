// rwr_render — headless counterpart of the reference's `run()` event loop
// (/root/reference/src/lib.rs:1233-1352, src/main.rs): State::new, then per frame
// input* -> update -> render, with key events taken from a script instead of a window.
//
//   rwr_render --res DIR [--scene suzanne_lowpoly.obj] [--size 600x600] [--keys "S*15,D*4"]
//              [--frames N] [--resize WxH@FRAME]... [--spp N] [--bounces B] [--accumulate] [--shadows] [--soft-shadows R[,R2]]
//              [--denoise [--denoise-iterations N] [--denoise-sigma S]] [--sky [--sky-zenith r,g,b] [--sky-horizon r,g,b]]
//              [--mirror-part N[:r,g,b]]... [--mirror-sphere N[:r,g,b]]... [--glass-part N[:ior[:r,g,b]]]...
//              [--glass-sphere N[:ior[:r,g,b]]]... [--gloss-part N:rough[:r,g,b]]... [--gloss-sphere N:rough[:r,g,b]]... [--reproject [--reproject-history N] [--reproject-normal C] [--reproject-depth X]]
//              [--emissive-part N:r,g,b]... [--emissive-sphere N:r,g,b]... [--light-sampling] [--light-parts] [--light-mis] [--sobol]
//              [--sky-image FILE[:scale] [--sky-image-size N]] [--light-sky]
//              [--tonemap [clamp|reinhard|aces]] [--exposure STOPS] [--auto-exposure [KEY]] [--white W] [--show-params] [--out frame.png] [--time]
//
// --keys: comma separated KEY*COUNT; each entry holds KEY down for COUNT frames
// (KEY in W A S D Up Down Left Right Space LShift, or '-' for no key).  After the script,
// --frames more frames are rendered with no key held.  The window default is 600x600
// (lib.rs:1248-1251).  --resize WxH@FRAME (repeatable): a WindowEvent::Resized delivered before frame FRAME
// (0-based, counted over the whole run) -> State::resize (lib.rs:772-989, 1323-1330), including its quirk: the
// camera's aspect is recomputed from the size BEFORE the resize.  --accumulate (extension): every frame sets
// RWR_FLAG_ACCUMULATE, so the image converges while the camera rests (any change starts over); the program prints
// `samples N` for the final frame.  --reproject (extension): every frame sets RWR_FLAG_REPROJECT, so every frame — every key step's
// too — is blended with the history of the frames before it while the camera moves; the program prints `history K` for the
// final frame.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "image_codec.hpp"
#include "state.hpp"

using namespace rwr;

static VirtualKeyCode parse_key(const std::string &k)
{
    if (k == "W") return VirtualKeyCode::W;
    if (k == "A") return VirtualKeyCode::A;
    if (k == "S") return VirtualKeyCode::S;
    if (k == "D") return VirtualKeyCode::D;
    if (k == "Up") return VirtualKeyCode::Up;
    if (k == "Down") return VirtualKeyCode::Down;
    if (k == "Left") return VirtualKeyCode::Left;
    if (k == "Right") return VirtualKeyCode::Right;
    if (k == "Space") return VirtualKeyCode::Space;
    if (k == "LShift") return VirtualKeyCode::LShift;
    return VirtualKeyCode::Other;
}

int main(int argc, char **argv)
{
    std::string res, scene = "suzanne_lowpoly.obj", out, keys;
    uint32_t w = 600, h = 600, frames = 1, spp = 1, bounces = 0;
    bool timing = false, accumulate = false, shadows = false, denoise = false;
    int denoise_iterations = 0;      // 0: the library's default
    float denoise_sigma = 0.0f;      // 0: the library's default
    bool reproject = false, reproject_set = false;
    rwr_reproject_params reproject_params{32u, 0.95f, 0.05f};   // the library's defaults
    // a number and nothing else (no "nan", no "inf", no trailing text)
    auto parse_number = [](const char *text, double &out) {
        if (!((*text >= '0' && *text <= '9') || *text == '.' || *text == '-' || *text == '+')) return false;
        char *end = nullptr;
        out = std::strtod(text, &end);
        return end != text && *end == '\0' && out == out && out - out == 0.0;
    };
    bool soft_shadows = false;
    rwr_shadow_params shadow_params = RWR_SHADOW_DEFAULTS;   // the library's defaults
    bool sky = false, sky_zenith_set = false, sky_horizon_set = false, show_params = false;
    rwr_sky_params sky_params = RWR_SKY_DEFAULTS;   // the library's defaults
    // "r,g,b": three numbers and nothing else, each finite and in [0, 16] (rwr_sky_set_params' range)
    auto parse_colour = [](const char *text, float out[3]) {
        float v[3];
        char tail = 0;
        if (std::sscanf(text, "%f,%f,%f%c", &v[0], &v[1], &v[2], &tail) != 3) return false;
        for (int c = 0; c < 3; c++)
            if (!(v[c] >= 0.0f && v[c] <= RWR_SKY_COMPONENT_MAX)) return false;
        for (int c = 0; c < 3; c++) out[c] = v[c];
        return true;
    };
    // --mirror-part / --mirror-sphere "N" or "N:r,g,b": an index and a reflectance in [0, 1]^3 (1,1,1 when left out)
    struct Mirror { bool sphere; uint32_t index; float r[3]; };
    std::vector<Mirror> mirrors;
    auto parse_mirror = [](const char *text, Mirror &m) {
        char *end = nullptr;
        if (*text < '0' || *text > '9') return false;
        const unsigned long idx = std::strtoul(text, &end, 10);
        if (end == text || idx > 0xfffffffful) return false;
        m.index = (uint32_t)idx;
        m.r[0] = m.r[1] = m.r[2] = 1.0f;
        if (*end == '\0') return true;
        if (*end != ':') return false;
        float v[3];
        char tail = 0;
        if (std::sscanf(end + 1, "%f,%f,%f%c", &v[0], &v[1], &v[2], &tail) != 3) return false;
        for (int c = 0; c < 3; c++)
            if (!(v[c] >= 0.0f && v[c] <= 1.0f)) return false;
        for (int c = 0; c < 3; c++) m.r[c] = v[c];
        return true;
    };
    // --glass-part / --glass-sphere "N", "N:ior" or "N:ior:r,g,b": an index, an index of refraction in [1, 4] (1.5 when left out)
    // and a tint in [0, 1]^3 (1,1,1 when left out)
    struct Glass { bool sphere; uint32_t index; float ior; float tint[3]; };
    std::vector<Glass> glasses;
    auto parse_glass = [](const char *text, Glass &g) {
        char *end = nullptr;
        if (*text < '0' || *text > '9') return false;
        const unsigned long idx = std::strtoul(text, &end, 10);
        if (end == text || idx > 0xfffffffful) return false;
        g.index = (uint32_t)idx;
        g.ior = 1.5f;
        g.tint[0] = g.tint[1] = g.tint[2] = 1.0f;
        if (*end == '\0') return true;
        if (*end != ':') return false;
        const char *ior_text = end + 1;
        if (!((*ior_text >= '0' && *ior_text <= '9') || *ior_text == '.')) return false;   // (no sign, no "nan", no "inf")
        const float ior = std::strtof(ior_text, &end);
        if (end == ior_text || !(ior >= 1.0f && ior <= 4.0f)) return false;
        g.ior = ior;
        if (*end == '\0') return true;
        if (*end != ':') return false;
        float v[3];
        char tail = 0;
        if (std::sscanf(end + 1, "%f,%f,%f%c", &v[0], &v[1], &v[2], &tail) != 3) return false;
        for (int c = 0; c < 3; c++)
            if (!(v[c] >= 0.0f && v[c] <= 1.0f)) return false;
        for (int c = 0; c < 3; c++) g.tint[c] = v[c];
        return true;
    };
    // --gloss-part / --gloss-sphere "N:rough" or "N:rough:r,g,b": an index, a roughness in [2^-10, 1] and a reflectance in [0, 1]^3
    // (1,1,1 when left out)
    struct Gloss { bool sphere; uint32_t index; float rough; float r[3]; };
    std::vector<Gloss> glosses;
    auto parse_gloss = [](const char *text, Gloss &g) {
        char *end = nullptr;
        if (*text < '0' || *text > '9') return false;
        const unsigned long idx = std::strtoul(text, &end, 10);
        if (end == text || idx > 0xfffffffful) return false;
        g.index = (uint32_t)idx;
        g.r[0] = g.r[1] = g.r[2] = 1.0f;
        if (*end != ':') return false;   // (the roughness is not optional: a surface without one is a mirror)
        const char *rough_text = end + 1;
        if (!((*rough_text >= '0' && *rough_text <= '9') || *rough_text == '.')) return false;   // (no sign, no "nan", no "inf")
        const float rough = std::strtof(rough_text, &end);
        if (end == rough_text || !(rough >= 0x1p-10f && rough <= 1.0f)) return false;
        g.rough = rough;
        if (*end == '\0') return true;
        if (*end != ':') return false;
        float v[3];
        char tail = 0;
        if (std::sscanf(end + 1, "%f,%f,%f%c", &v[0], &v[1], &v[2], &tail) != 3) return false;
        for (int c = 0; c < 3; c++)
            if (!(v[c] >= 0.0f && v[c] <= 1.0f)) return false;
        for (int c = 0; c < 3; c++) g.r[c] = v[c];
        return true;
    };
    // --emissive-part / --emissive-sphere "N:r,g,b": an index and a radiance in [0, RWR_MAX_EMISSION]^3
    struct Emitter { bool sphere; uint32_t index; float le[3]; };
    std::vector<Emitter> emitters;
    bool light_sampling = false;   // --light-sampling
    bool light_parts = false;      // --light-parts
    bool light_mis = false;        // --light-mis
    bool light_sky = false;        // --light-sky
    bool sobol = false;            // --sobol
    auto parse_emitter = [](const char *text, Emitter &e) {
        char *end = nullptr;
        if (*text < '0' || *text > '9') return false;
        const unsigned long idx = std::strtoul(text, &end, 10);
        if (end == text || idx > 0xfffffffful || *end != ':') return false;
        e.index = (uint32_t)idx;
        float v[3];
        char tail = 0;
        if (std::sscanf(end + 1, "%f,%f,%f%c", &v[0], &v[1], &v[2], &tail) != 3) return false;
        for (int c = 0; c < 3; c++)   // (false for NaN)
            if (!(v[c] >= 0.0f && v[c] <= RWR_MAX_EMISSION)) return false;
        for (int c = 0; c < 3; c++) e.le[c] = v[c];
        return true;
    };
    // --sky-image FILE[:scale] [--sky-image-size N]: a latitude-longitude picture for RWR_FLAG_SKY_IMAGE, its scale and the map's side
    std::string sky_image;
    double sky_image_scale = 1.0;
    uint32_t sky_image_size = 256u;
    struct Resize { uint64_t frame; uint32_t w, h; };
    std::vector<Resize> resizes;
    // --tonemap [CURVE], --exposure STOPS, --auto-exposure [KEY], --white W: RWR_FLAG_TONEMAP and its parameters (the library's defaults)
    bool tonemap = false;
    rwr_tonemap_params tonemap_params = RWR_TONEMAP_DEFAULTS;
    const char *const curve_names[3] = {"clamp", "reinhard", "aces"};
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char * {
            if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); }
            return argv[++i];
        };
        // the value of an option that may stand without one: the next argument unless it is an option itself (null: none)
        auto next_optional = [&]() -> const char * {
            if (i + 1 >= argc || std::strncmp(argv[i + 1], "--", 2) == 0) return nullptr;
            return argv[++i];
        };
        if (a == "--res") res = next();
        else if (a == "--scene") scene = next();
        else if (a == "--out") out = next();
        else if (a == "--keys") keys = next();
        else if (a == "--frames") frames = (uint32_t)std::atoi(next());
        else if (a == "--spp") spp = (uint32_t)std::atoi(next());
        else if (a == "--bounces") bounces = (uint32_t)std::atoi(next());
        else if (a == "--time") timing = true;
        else if (a == "--accumulate") accumulate = true;
        else if (a == "--shadows") shadows = true;
        else if (a == "--soft-shadows") {   // "R" (both lights) or "R,R2" (the mesh shader's light, the sphere shader's): numbers in [0, 1]
            const std::string v = next();
            const size_t comma = v.find(',');
            double r0 = 0.0, r1 = 0.0;
            bool ok = parse_number(v.substr(0, comma).c_str(), r0);
            r1 = r0;
            if (ok && comma != std::string::npos) ok = parse_number(v.c_str() + comma + 1, r1);
            if (!ok || r0 < 0.0 || r0 > (double)RWR_SHADOW_RADIUS_MAX || r1 < 0.0 || r1 > (double)RWR_SHADOW_RADIUS_MAX) {
                std::fprintf(stderr, "--soft-shadows R[,R2]: one or two numbers in [0, 1]\n");
                return 2;
            }
            shadow_params.mesh_light_radius = (float)r0;
            shadow_params.sphere_light_radius = (float)r1;
            shadows = soft_shadows = true;
        }
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-iterations") { denoise = true; denoise_iterations = std::atoi(next()); }
        else if (a == "--denoise-sigma") { denoise = true; denoise_sigma = (float)std::atof(next()); }
        else if (a == "--tonemap") {
            tonemap = true;
            if (const char *v = next_optional()) {
                uint32_t c = 0;
                while (c < 3u && std::strcmp(v, curve_names[c]) != 0) c++;
                if (c == 3u) { std::fprintf(stderr, "--tonemap [clamp|reinhard|aces]: '%s' is none of them\n", v); return 2; }
                tonemap_params.curve = c;
            }
        }
        else if (a == "--exposure") {   // stops: the factor is 2^STOPS, computed in double
            double v = 0.0;
            if (!parse_number(next(), v) || v < -16.0 || v > 16.0) { std::fprintf(stderr, "--exposure STOPS: a number in [-16, 16]\n"); return 2; }
            tonemap_params.exposure = (float)std::exp2(v);
            tonemap = true;
        }
        else if (a == "--auto-exposure") {
            tonemap = true;
            tonemap_params.auto_exposure = 1u;
            if (const char *text = next_optional()) {
                double v = 0.0;
                if (!parse_number(text, v) || v < 1.0 / 65536.0 || v > 65536.0) { std::fprintf(stderr, "--auto-exposure [KEY]: a number in [2^-16, 2^16]\n"); return 2; }
                tonemap_params.key = (float)v;
            }
        }
        else if (a == "--white") {
            double v = 0.0;
            if (!parse_number(next(), v) || v < 1.0 / 256.0 || v > 65536.0) { std::fprintf(stderr, "--white W: a number in [2^-8, 2^16]\n"); return 2; }
            tonemap_params.white = (float)v;
            tonemap = true;
        }
        else if (a == "--reproject") reproject = true;
        else if (a == "--reproject-history" || a == "--reproject-normal" || a == "--reproject-depth") {
            double v = 0.0;
            const bool ok = parse_number(next(), v);
            if (a == "--reproject-history") {
                if (!ok || v != (double)(uint32_t)v || v < 1.0 || v > 1024.0) { std::fprintf(stderr, "--reproject-history N: a whole number in [1, 1024]\n"); return 2; }
                reproject_params.max_history = (uint32_t)v;
            } else if (a == "--reproject-normal") {
                if (!ok || v < -1.0 || v > 1.0) { std::fprintf(stderr, "--reproject-normal C: a number in [-1, 1]\n"); return 2; }
                reproject_params.normal_cos_min = (float)v;
            } else {
                if (!ok || v < 0.0 || !((float)v - (float)v == 0.0f)) { std::fprintf(stderr, "--reproject-depth X: a finite number >= 0\n"); return 2; }
                reproject_params.depth_rel = (float)v;
            }
            reproject = reproject_set = true;
        }
        else if (a == "--sky") sky = true;
        else if (a == "--sky-zenith" || a == "--sky-horizon") {
            const bool zenith = a == "--sky-zenith";
            if (!parse_colour(next(), zenith ? sky_params.zenith : sky_params.horizon)) {
                std::fprintf(stderr, "%s r,g,b: three numbers in [0, 16]\n", a.c_str());
                return 2;
            }
            sky = true;
            (zenith ? sky_zenith_set : sky_horizon_set) = true;
        }
        else if (a == "--sky-image") {   // "FILE" or "FILE:scale", the scale a finite number >= 0 behind the last colon
            sky_image = next();
            const size_t colon = sky_image.rfind(':');
            double v = 0.0;
            if (colon != std::string::npos && colon + 1 < sky_image.size() && sky_image.find('/', colon) == std::string::npos) {
                if (!parse_number(sky_image.c_str() + colon + 1, v) || v < 0.0 || !((float)v - (float)v == 0.0f)) {
                    std::fprintf(stderr, "--sky-image FILE[:scale]: the scale is a finite number >= 0\n");
                    return 2;
                }
                sky_image_scale = v;
                sky_image.resize(colon);
            }
            if (sky_image.empty()) { std::fprintf(stderr, "--sky-image FILE[:scale]: no file\n"); return 2; }
            sky = true;
        }
        else if (a == "--sky-image-size") {
            double v = 0.0;
            if (!parse_number(next(), v) || v != (double)(uint32_t)v || v < 2.0 || v > (double)RWR_SKY_IMAGE_SIZE_MAX) {
                std::fprintf(stderr, "--sky-image-size N: a whole number in [2, %u]\n", RWR_SKY_IMAGE_SIZE_MAX);
                return 2;
            }
            sky_image_size = (uint32_t)v;
        }
        else if (a == "--mirror-part" || a == "--mirror-sphere") {
            Mirror m{a == "--mirror-sphere", 0u, {1.0f, 1.0f, 1.0f}};
            if (!parse_mirror(next(), m) || (m.sphere && m.index >= RWR_MAX_SPHERES)) {
                std::fprintf(stderr, "%s N[:r,g,b]: an index%s and three numbers in [0, 1]\n", a.c_str(), m.sphere ? " below 8" : "");
                return 2;
            }
            mirrors.push_back(m);
        }
        else if (a == "--glass-part" || a == "--glass-sphere") {
            Glass g{a == "--glass-sphere", 0u, 1.5f, {1.0f, 1.0f, 1.0f}};
            if (!parse_glass(next(), g) || (g.sphere && g.index >= RWR_MAX_SPHERES)) {
                std::fprintf(stderr, "%s N[:ior[:r,g,b]]: an index%s, an index of refraction in [1, 4] and three numbers in [0, 1]\n", a.c_str(),
                             g.sphere ? " below 8" : "");
                return 2;
            }
            glasses.push_back(g);
        }
        else if (a == "--gloss-part" || a == "--gloss-sphere") {
            Gloss g{a == "--gloss-sphere", 0u, 0.25f, {1.0f, 1.0f, 1.0f}};
            if (!parse_gloss(next(), g) || (g.sphere && g.index >= RWR_MAX_SPHERES)) {
                std::fprintf(stderr, "%s N:rough[:r,g,b]: an index%s, a roughness in [2^-10, 1] and three numbers in [0, 1]\n", a.c_str(),
                             g.sphere ? " below 8" : "");
                return 2;
            }
            glosses.push_back(g);
        }
        else if (a == "--emissive-part" || a == "--emissive-sphere") {
            Emitter e{a == "--emissive-sphere", 0u, {0.0f, 0.0f, 0.0f}};
            if (!parse_emitter(next(), e) || (e.sphere && e.index >= RWR_MAX_SPHERES)) {
                std::fprintf(stderr, "%s N:r,g,b: an index%s and three numbers in [0, %g]\n", a.c_str(), e.sphere ? " below 8" : "", (double)RWR_MAX_EMISSION);
                return 2;
            }
            emitters.push_back(e);
        }
        else if (a == "--light-sampling") light_sampling = true;
        else if (a == "--light-parts") light_parts = true;
        else if (a == "--light-mis") light_mis = true;
        else if (a == "--light-sky") light_sky = true;
        else if (a == "--sobol") sobol = true;
        else if (a == "--show-params") show_params = true;
        else if (a == "--resize") {
            Resize r{0, 0, 0};
            unsigned long long f = 0;
            if (std::sscanf(next(), "%ux%u@%llu", &r.w, &r.h, &f) != 3) { std::fprintf(stderr, "--resize WxH@FRAME\n"); return 2; }
            r.frame = f;
            resizes.push_back(r);
        }
        else if (a == "--size") {
            if (std::sscanf(next(), "%ux%u", &w, &h) != 2) { std::fprintf(stderr, "--size WxH\n"); return 2; }
        } else if (a == "--help" || a == "-h") {
            std::printf("usage: rwr_render --res DIR [--scene F.obj] [--size WxH] [--keys \"S*15,D*4\"] [--frames N] "
                        "[--resize WxH@FRAME]... [--spp N] [--bounces B] [--accumulate] [--shadows] [--soft-shadows R[,R2]] "
                        "[--denoise [--denoise-iterations N] [--denoise-sigma S]] [--sky [--sky-zenith r,g,b] [--sky-horizon r,g,b]] "
                        "[--mirror-part N[:r,g,b]]... [--mirror-sphere N[:r,g,b]]... [--glass-part N[:ior[:r,g,b]]]... "
                        "[--glass-sphere N[:ior[:r,g,b]]]... [--gloss-part N:rough[:r,g,b]]... [--gloss-sphere N:rough[:r,g,b]]... "
                        "[--emissive-part N:r,g,b]... [--emissive-sphere N:r,g,b]... [--light-sampling] [--light-parts] [--light-mis] [--sobol] [--sky-image FILE[:scale] [--sky-image-size N]] [--light-sky] "
                        "[--reproject [--reproject-history N] [--reproject-normal C] [--reproject-depth X]] "
                        "[--tonemap [clamp|reinhard|aces]] [--exposure STOPS] [--auto-exposure [KEY]] [--white W] "
                        "[--show-params] [--out frame.png] [--time]\n"
                        "  --accumulate  every frame adds its samples to those of the frames before while nothing changes "
                        "(RWR_FLAG_ACCUMULATE); prints `samples N` for the final frame\n"
                        "  --shadows     every hit casts a shadow ray towards its light (RWR_FLAG_SHADOWS); works with --spp, --bounces "
                        "and --accumulate\n"
                        "  --soft-shadows R[,R2]  the two lights get an angular size, so that shadows get penumbrae (RWR_FLAG_SOFT_SHADOWS; implies "
                        "--shadows): R is the tangent of the half-angle a hit sees the light under, in [0, 1] (0.0047: the sun; 0: the point light "
                        "of --shadows); one value sets both lights, two the mesh shader's and the sphere shader's (rwr_shadow_set_params)\n"
                        "  --denoise     the edge-avoiding a-trous filter over every frame (RWR_FLAG_DENOISE): N iterations (1-5), colour "
                        "sigma S (rwr_denoise_set_params)\n"
                        "  --sky         bounce rays that leave the scene return the sky's radiance (RWR_FLAG_SKY; needs --bounces >= 1): a "
                        "gradient from --sky-horizon (straight down) to --sky-zenith (straight up), components in [0, 16] "
                        "(rwr_sky_set_params); either colour implies --sky\n"
                        "  --sky-image FILE[:scale]  the sky's radiance comes from a picture of a place instead of the gradient "
                        "(RWR_FLAG_SKY_IMAGE; implies --sky): a latitude-longitude PNG or JPEG (taken to linear) or a Radiance .hdr file, top row "
                        "straight up, the centre column towards -z; multiplied by scale (1 when left out; an 8-bit picture wants about 4 to "
                        "light a scene), converted to an octahedral map of --sky-image-size N texels a side (256 when left out; 2 ... 2048) "
                        "(rwr_sky_image_from_equirect, rwr_sky_set_image)\n"
                        "  --mirror-part N[:r,g,b], --mirror-sphere N[:r,g,b]  part N of the scene / sphere N is a mirror of reflectance r,g,b "
                        "in [0, 1] (1,1,1 when left out) and reflects the ray that found it (RWR_FLAG_MIRRORS, implied; needs --bounces >= 1; "
                        "rwr_scene_set_part_mirror / rwr_scene_set_sphere_mirror); repeatable\n"
                        "  --glass-part N[:ior[:r,g,b]], --glass-sphere N[:ior[:r,g,b]]  part N of the scene / sphere N is glass of index of "
                        "refraction ior in [1, 4] (1.5 when left out) and tint r,g,b in [0, 1] (1,1,1 when left out): it reflects by Fresnel's law and "
                        "refracts by Snell's (RWR_FLAG_GLASS, implied; needs --bounces >= 1, and several for a ray to get through; "
                        "rwr_scene_set_part_glass / rwr_scene_set_sphere_glass); repeatable\n"
                        "  --gloss-part N:rough[:r,g,b], --gloss-sphere N:rough[:r,g,b]  part N of the scene / sphere N is glossy, of roughness rough "
                        "in [2^-10, 1] (towards 0 a mirror, 1 diffuse) and reflectance r,g,b in [0, 1] (1,1,1 when left out): it sends on a ray between "
                        "the mirror reflection and the diffuse ray (RWR_FLAG_GLOSSY, implied; needs --bounces >= 1; rwr_scene_set_part_gloss / "
                        "rwr_scene_set_sphere_gloss); repeatable; prints `glossy rays N` for the final frame.  Mirror, glass and gloss options "
                        "are applied in that order: of several for one surface the last of these wins\n"
                        "  --emissive-part N:r,g,b, --emissive-sphere N:r,g,b  part N of the scene / sphere N gives off light of radiance r,g,b in "
                        "[0, 64], whatever its surface model (RWR_FLAG_EMISSIVE, implied; rwr_scene_set_part_emission / "
                        "rwr_scene_set_sphere_emission); repeatable; prints `emissive hits N` for the final frame.  A ray is aimed at an emitting "
                        "sphere with --light-sampling alone and at an emitting part with --light-parts alone: without them a small lamp wants many samples\n"
                        "  --light-sampling  every diffuse hit also sends a ray towards an emitting sphere (RWR_FLAG_LIGHT_SAMPLING; implies "
                        "nothing: it needs --emissive-sphere and --bounces >= 1 to do anything); prints `light rays N, reached M` for the final frame\n"
                        "  --light-parts  every diffuse hit's light ray may aim at a point on a face of an emitting part (RWR_FLAG_LIGHT_PARTS; implies "
                        "nothing: it needs --emissive-part and --bounces >= 1 to do anything; with --light-sampling one ray per hit chooses among "
                        "the spheres and the parts); prints `part light rays N, reached M` for the final frame\n"
                        "  --light-mis  the light ray and the diffuse bounce ray that finds the same emitter are combined by the balance heuristic "
                        "(RWR_FLAG_LIGHT_MIS, multiple importance sampling; implies nothing: it needs --light-sampling or --light-parts in effect to do "
                        "anything); with it both may stay on in a scene that glows all over; prints `weighted hits N` for the final frame\n"
                        "  --light-sky   every diffuse hit's light ray may aim at the sky's image, drawn in proportion to its radiance "
                        "(RWR_FLAG_LIGHT_SKY; implies nothing: it needs --sky-image, --sky and --bounces >= 1 to do anything; with the other light "
                        "flags one ray per hit chooses among the spheres, the parts and the sky; best with --light-mis): a picture with a small sun "
                        "converges; prints `sky light rays N, reached M` for the final frame\n"
                        "  --sobol       every random number of the path tracer comes from an Owen-scrambled Sobol sequence instead of the "
                        "independent hash (RWR_FLAG_SOBOL; implies nothing: it does something in frames with --spp > 1, --bounces >= 1, "
                        "--accumulate or --soft-shadows): a pixel's samples are stratified against each other, so that 16 samples "
                        "give about the error of 64\n"
                        "  --reproject   every frame is blended with the history of the frames before it, fetched where its points were seen "
                        "last frame, while the camera moves (RWR_FLAG_REPROJECT; with --keys every key step's frame feeds the next one's history): "
                        "at most N frames of history per pixel (1-1024), taps of faces whose normals' cosine is at least C and whose distance "
                        "differs by at most X of itself (rwr_reproject_set_params); a value implies --reproject; prints `history K` for the final frame\n"
                        "  --tonemap [clamp|reinhard|aces]  the picture is curve(exposure x radiance) instead of the radiance cut off at 1, so that a "
                        "lamp and the wall beside it keep apart (RWR_FLAG_TONEMAP; aces when left out; rwr_tonemap_set_params).  --exposure STOPS: "
                        "the factor 2^STOPS, STOPS in [-16, 16]; --auto-exposure [KEY]: the exposure that brings the frame's log-average luminance, "
                        "measured on the GPU, to KEY (0.18 when left out), times --exposure's factor; --white W: the radiance Reinhard's curve maps "
                        "to 1 (4 when left out).  Each of the three implies --tonemap; prints `exposure E (log-average G over N pixels)` for the "
                        "final frame\n"
                        "  --show-params prints the render parameters the arguments give and exits, without a device\n");
            return 0;
        } else {
            std::fprintf(stderr, "unknown argument %s\n", a.c_str());
            return 2;
        }
    }
    const uint32_t flags = (accumulate ? (uint32_t)RWR_FLAG_ACCUMULATE : 0u) | (bounces > 1u ? (uint32_t)RWR_FLAG_MULTI_BOUNCE : 0u) |   // more than one bounce: the deeper paths
                           (shadows ? (uint32_t)RWR_FLAG_SHADOWS : 0u) | (denoise ? (uint32_t)RWR_FLAG_DENOISE : 0u) | (sky ? (uint32_t)RWR_FLAG_SKY : 0u) |
                           (mirrors.empty() ? 0u : (uint32_t)RWR_FLAG_MIRRORS) | (glasses.empty() ? 0u : (uint32_t)RWR_FLAG_GLASS) |
                           (glosses.empty() ? 0u : (uint32_t)RWR_FLAG_GLOSSY) | (soft_shadows ? (uint32_t)RWR_FLAG_SOFT_SHADOWS : 0u) |
                           (reproject ? (uint32_t)RWR_FLAG_REPROJECT : 0u) | (emitters.empty() ? 0u : (uint32_t)RWR_FLAG_EMISSIVE) |
                           (light_sampling ? (uint32_t)RWR_FLAG_LIGHT_SAMPLING : 0u) | (light_parts ? (uint32_t)RWR_FLAG_LIGHT_PARTS : 0u) |
                           (light_mis ? (uint32_t)RWR_FLAG_LIGHT_MIS : 0u) | (sobol ? (uint32_t)RWR_FLAG_SOBOL : 0u) |
                           (sky_image.empty() ? 0u : (uint32_t)RWR_FLAG_SKY_IMAGE) | (light_sky ? (uint32_t)RWR_FLAG_LIGHT_SKY : 0u) |
                           (tonemap ? (uint32_t)RWR_FLAG_TONEMAP : 0u);
    if (show_params) {
        if (tonemap)   // (a line of its own, ahead of the line every run prints)
            std::printf("tonemap 1 curve %s auto-exposure %u exposure %g key %g white %g\n", curve_names[tonemap_params.curve], tonemap_params.auto_exposure,
                        (double)tonemap_params.exposure, (double)tonemap_params.key, (double)tonemap_params.white);
        if (reproject)   // (a line of its own, ahead of the line every run prints)
            std::printf("reproject 1 history %u normal %g depth %g\n", reproject_params.max_history, (double)reproject_params.normal_cos_min,
                        (double)reproject_params.depth_rel);
        if (soft_shadows)   // (likewise)
            std::printf("soft-shadows 1 radii %g,%g\n", (double)shadow_params.mesh_light_radius, (double)shadow_params.sphere_light_radius);
        if (!emitters.empty()) {   // (likewise)
            std::printf("emissive %zu", emitters.size());
            for (const Emitter &e : emitters)
                std::printf(" %s %u:%g,%g,%g", e.sphere ? "sphere" : "part", e.index, (double)e.le[0], (double)e.le[1], (double)e.le[2]);
            std::printf("\n");
        }
        if (!sky_image.empty())   // (likewise)
            std::printf("sky image %u scale %g file %s\n", sky_image_size, sky_image_scale, sky_image.c_str());
        std::printf("spp %u bounces %u flags 0x%x sky %d zenith %g,%g,%g horizon %g,%g,%g gloss %zu", spp, bounces, flags, sky ? 1 : 0,
                    (double)sky_params.zenith[0], (double)sky_params.zenith[1], (double)sky_params.zenith[2],
                    (double)sky_params.horizon[0], (double)sky_params.horizon[1], (double)sky_params.horizon[2], glosses.size());
        for (const Gloss &g : glosses)
            std::printf(" %s %u:%g:%g,%g,%g", g.sphere ? "sphere" : "part", g.index, (double)g.rough, (double)g.r[0], (double)g.r[1], (double)g.r[2]);
        std::printf(" glass %zu", glasses.size());
        for (const Glass &g : glasses)
            std::printf(" %s %u:%g:%g,%g,%g", g.sphere ? "sphere" : "part", g.index, (double)g.ior, (double)g.tint[0], (double)g.tint[1], (double)g.tint[2]);
        std::printf(" mirrors %zu", mirrors.size());
        for (const Mirror &m : mirrors)
            std::printf(" %s %u:%g,%g,%g", m.sphere ? "sphere" : "part", m.index, (double)m.r[0], (double)m.r[1], (double)m.r[2]);
        std::printf("\n");
        return 0;
    }
    if (res.empty()) { std::fprintf(stderr, "--res DIR is required (the reference bakes OUT_DIR/res in at compile time)\n"); return 2; }

    // script: (key, frames held)
    std::vector<std::pair<VirtualKeyCode, uint32_t>> script;
    size_t pos = 0;
    while (pos < keys.size()) {
        const size_t comma = keys.find(',', pos);
        const std::string item = keys.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
        const size_t star = item.find('*');
        const std::string k = item.substr(0, star);
        const uint32_t n = star == std::string::npos ? 1u : (uint32_t)std::atoi(item.c_str() + star + 1);
        if (k != "-" && parse_key(k) == VirtualKeyCode::Other) { std::fprintf(stderr, "unknown key '%s'\n", k.c_str()); return 2; }
        script.emplace_back(parse_key(k), n);
        if (comma == std::string::npos) break;
        pos = comma + 1;
    }

    // the sky's picture, decoded and converted ahead of the device: PNG / JPEG through the texture path's decoders and the sRGB
    // curve, .hdr as it stands
    std::vector<float> sky_map;
    if (!sky_image.empty()) {
        std::vector<uint8_t> bytes;
        if (FILE *f = std::fopen(sky_image.c_str(), "rb")) {
            uint8_t buf[65536];
            for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) != 0;) bytes.insert(bytes.end(), buf, buf + got);
            std::fclose(f);
        } else {
            std::fprintf(stderr, "--sky-image: cannot open %s\n", sky_image.c_str());
            return 2;
        }
        codec::ImageF pic;
        std::string err;
        if (codec::is_hdr(bytes.data(), bytes.size())) {
            if (!codec::decode_hdr(bytes.data(), bytes.size(), pic, err)) { std::fprintf(stderr, "--sky-image: %s: %s\n", sky_image.c_str(), err.c_str()); return 2; }
        } else {
            codec::Image ldr;
            if (!codec::decode_image(bytes.data(), bytes.size(), ldr, err)) { std::fprintf(stderr, "--sky-image: %s: %s\n", sky_image.c_str(), err.c_str()); return 2; }
            float lut[256];
            for (int i = 0; i < 256; i++) {
                const double c = i / 255.0;
                lut[i] = (float)(c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4));
            }
            pic.width = ldr.width; pic.height = ldr.height;
            pic.rgb.resize((size_t)ldr.width * ldr.height * 3u);
            for (size_t i = 0; i < (size_t)ldr.width * ldr.height; i++)
                for (int c = 0; c < 3; c++) pic.rgb[3u * i + c] = lut[ldr.rgba[4u * i + c]];
        }
        sky_map.resize((size_t)sky_image_size * sky_image_size * 3u);
        if (rwr_sky_image_from_equirect(pic.rgb.data(), pic.width, pic.height, (float)sky_image_scale, sky_image_size, sky_map.data()) != RWR_OK) {
            std::fprintf(stderr, "--sky-image: %s\n", rwr_last_error_string());
            return 2;
        }
    }

    try {
        State state(w, h, res, scene);
        const rwr_render_params params{spp, bounces, 0u, flags};
        if (sky_zenith_set || sky_horizon_set) {
            if (rwr_sky_set_params(state.context(), &sky_params) != RWR_OK) { std::fprintf(stderr, "--sky: %s\n", rwr_last_error_string()); return 2; }
        }
        if (!sky_map.empty()) {
            if (rwr_sky_set_image(state.context(), sky_map.data(), sky_image_size) != RWR_OK) { std::fprintf(stderr, "--sky-image: %s\n", rwr_last_error_string()); return 2; }
        }
        if (soft_shadows) state.set_shadow_params(shadow_params);   // (in range already: a failure is the library's, reported below)
        for (const Mirror &m : mirrors) {   // (the scene is loaded: a part the scene does not have is the library's refusal)
            const int rc = m.sphere ? rwr_scene_set_sphere_mirror(state.context(), m.index, m.r) : rwr_scene_set_part_mirror(state.context(), m.index, m.r);
            if (rc != RWR_OK) { std::fprintf(stderr, "%s: %s\n", m.sphere ? "--mirror-sphere" : "--mirror-part", rwr_last_error_string()); return 2; }
        }
        for (const Glass &g : glasses) {   // (after the mirrors: a surface has one model, the later option wins)
            const int rc = g.sphere ? rwr_scene_set_sphere_glass(state.context(), g.index, g.ior, g.tint) : rwr_scene_set_part_glass(state.context(), g.index, g.ior, g.tint);
            if (rc != RWR_OK) { std::fprintf(stderr, "%s: %s\n", g.sphere ? "--glass-sphere" : "--glass-part", rwr_last_error_string()); return 2; }
        }
        for (const Gloss &g : glosses) {   // (after the mirrors and the glass: the later option wins)
            const int rc = g.sphere ? rwr_scene_set_sphere_gloss(state.context(), g.index, g.r, g.rough) : rwr_scene_set_part_gloss(state.context(), g.index, g.r, g.rough);
            if (rc != RWR_OK) { std::fprintf(stderr, "%s: %s\n", g.sphere ? "--gloss-sphere" : "--gloss-part", rwr_last_error_string()); return 2; }
        }
        for (const Emitter &e : emitters) {   // (beside the surface's model: no order among these and the three above)
            const int rc = e.sphere ? rwr_scene_set_sphere_emission(state.context(), e.index, e.le) : rwr_scene_set_part_emission(state.context(), e.index, e.le);
            if (rc != RWR_OK) { std::fprintf(stderr, "%s: %s\n", e.sphere ? "--emissive-sphere" : "--emissive-part", rwr_last_error_string()); return 2; }
        }
        if (denoise_iterations != 0 || denoise_sigma != 0.0f) {
            rwr_denoise_params dp;
            int rc = rwr_denoise_get_params(state.context(), &dp);
            if (denoise_iterations != 0) dp.iterations = (uint32_t)denoise_iterations;
            if (denoise_sigma != 0.0f) dp.sigma_color = denoise_sigma;
            if (rc == RWR_OK) rc = rwr_denoise_set_params(state.context(), &dp);
            if (rc != RWR_OK) { std::fprintf(stderr, "--denoise: %s\n", rwr_last_error_string()); return 2; }
        }
        if (reproject_set) {
            if (rwr_reproject_set_params(state.context(), &reproject_params) != RWR_OK) { std::fprintf(stderr, "--reproject: %s\n", rwr_last_error_string()); return 2; }
        }
        if (tonemap) {
            if (rwr_tonemap_set_params(state.context(), &tonemap_params) != RWR_OK) { std::fprintf(stderr, "--tonemap: %s\n", rwr_last_error_string()); return 2; }
        }
        uint64_t rendered = 0;
        const auto t0 = std::chrono::steady_clock::now();
        auto frame = [&]() {  // [Resized: resize()] then RedrawRequested: update() then render() (lib.rs:1323-1337)
            for (const Resize &r : resizes)
                if (r.frame == rendered) state.resize(r.w, r.h);
            state.update();
            state.render(&params);
            rendered++;
        };
        for (const auto &[key, n] : script) {
            if (key != VirtualKeyCode::Other) state.input(KeyboardInput{ElementState::Pressed, key});
            for (uint32_t f = 0; f < n; f++) frame();
            if (key != VirtualKeyCode::Other) state.input(KeyboardInput{ElementState::Released, key});
        }
        for (uint32_t f = 0; f < frames; f++) frame();
        check(rwr_synchronize(state.context()));
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const Camera &c = state.camera();
        std::printf("frames %llu  eye (%.6f, %.6f, %.6f)  target (%.6f, %.6f, %.6f)  size %ux%u  aspect %.9g\n", (unsigned long long)rendered,
                    c.eye.x, c.eye.y, c.eye.z, c.target.x, c.target.y, c.target.z, state.size().width, state.size().height, (double)c.aspect);
        if (!sky_map.empty()) std::printf("sky image %ux%u\n", sky_image_size, sky_image_size);
        if (accumulate) std::printf("samples %llu\n", (unsigned long long)state.accumulated_samples());
        if (reproject) std::printf("history %llu\n", (unsigned long long)state.reprojected_frames());
        if (!glosses.empty()) std::printf("glossy rays %llu\n", (unsigned long long)state.glossy_rays());
        if (!emitters.empty()) std::printf("emissive hits %llu\n", (unsigned long long)state.emissive_hits());
        if (light_sampling) {
            uint64_t rays = 0, reached = 0;
            state.light_rays(rays, reached);
            std::printf("light rays %llu, reached %llu\n", (unsigned long long)rays, (unsigned long long)reached);
        }
        if (light_parts) {
            uint64_t rays = 0, reached = 0;
            state.part_light_rays(rays, reached);
            std::printf("part light rays %llu, reached %llu\n", (unsigned long long)rays, (unsigned long long)reached);
        }
        if (light_sky) {
            uint64_t rays = 0, reached = 0;
            state.sky_light_rays(rays, reached);
            std::printf("sky light rays %llu, reached %llu\n", (unsigned long long)rays, (unsigned long long)reached);
        }
        if (tonemap) {   // G from the two sums as the flag's item 4 has it; a manual frame measured nothing
            int64_t log_sum = 0;
            uint32_t counted = 0;
            float E = 0.0f, G = 0.0f;
            check(rwr_last_tonemap_stats(state.context(), &log_sum, &counted, &E));
            if (counted) {
                int64_t m = log_sum / (int64_t)counted;
                if (log_sum % (int64_t)counted != 0 && log_sum < 0) m -= 1;
                const int32_t bits = 0x3f800000 + (int32_t)m;
                std::memcpy(&G, &bits, sizeof G);
            }
            std::printf("exposure %g (log-average %g over %u pixels)\n", (double)E, (double)G, counted);
        }
        if (light_mis) std::printf("weighted hits %llu\n", (unsigned long long)state.light_weighted_hits());
        if (timing) std::printf("%.3f ms/frame over %llu frames (update + render, host wall clock)\n", sec * 1e3 / (double)rendered,
                                (unsigned long long)rendered);
        if (!out.empty()) {
            state.present(out);
            std::printf("wrote %s (%ux%u, row 0 of the framebuffer at the bottom, sRGB encoded)\n", out.c_str(), state.size().width,
                        state.size().height);
        }
    } catch (const RwrFailure &e) {
        std::fprintf(stderr, "rwr_render: error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
