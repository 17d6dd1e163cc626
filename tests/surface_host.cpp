// csrc/rwr_surface.h for the host test (test_surface_decode_host.py): the kernels' decode_surface against the host's statement of a
// record's `on` - surface_model and surface_param - on every record a setter can store, under every set of surface flags.
#include <stdint.h>
#include <string.h>

#include "rwr_surface.h"

using namespace rwr;

namespace {

uint32_t bits_of(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}
float float_of(uint32_t u)
{
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

struct Tally {
    uint64_t checked = 0, bad = 0;
    uint32_t first_on = 0, first_modes = 0;   // the first disagreement: the stored `on` (its bits) and the frame's modes
};

// one record as a frame of `modes` sees it, read by the form SURF that frame runs
template <int SURF>
void check(float on, uint32_t modes, Tally &t)
{
    const SurfaceRec v = visible_record(SurfaceRec{0.25f, 0.5f, 0.75f, on}, modes);
    const SurfaceDecode d = decode_surface<SURF>(v.on);
    const SurfaceModel s = surface_model(v);
    const float param = surface_param(v);
    const bool model_ok = d.mirror == (s == SurfaceModel::kMirror) && d.glass == (s == SurfaceModel::kGlass) && d.gloss == (s == SurfaceModel::kGloss) &&
                          ((int)d.mirror + (int)d.glass + (int)d.gloss == (s == SurfaceModel::kDiffuse ? 0 : 1));
    const bool eta_ok = bits_of(d.eta) == bits_of(s == SurfaceModel::kGlass ? param : 0.0f);
    const bool rho_ok = bits_of(d.rho) == bits_of(s == SurfaceModel::kGloss ? param : 0.0f);
    t.checked++;
    if (!(model_ok && eta_ok && rho_ok)) {
        if (!t.bad) { t.first_on = bits_of(on); t.first_modes = modes; }
        t.bad++;
    }
}

void check_modes(float on, Tally &t)
{
    for (uint32_t modes = 1u; modes < 8u; modes++) {   // the seven sets of flags; SURF by WfFrame::surface_table's rule: gloss > glass > mirrors
        if (modes & surface_mode(SurfaceModel::kGloss)) check<kSurfGloss>(on, modes, t);
        else if (modes & surface_mode(SurfaceModel::kGlass)) check<kSurfGlass>(on, modes, t);
        else check<kSurfMirrors>(on, modes, t);
    }
}

}  // namespace

// out: {checks made, disagreements, first disagreeing `on` (bits), its modes, values of `on` covered}
extern "C" void surface_host_check(uint64_t out[5])
{
    Tally t;
    uint64_t values = 0;
    const float rgb[3] = {0.25f, 0.5f, 0.75f};
    check_modes(kDiffuseRec.on, t);
    check_modes(mirror_rec(rgb).on, t);
    values += 2;
    // glass: every float ior in [1, 4]
    for (uint32_t u = bits_of(kGlassIorMin); u <= bits_of(kGlassIorMax); u++, values++) check_modes(glass_rec(rgb, float_of(u)).on, t);
    // gloss: what 1 + roughness can round to for a roughness in [2^-10, 1] - every 1 + k 2^-23, k = 2^13 ... 2^23
    for (uint32_t k = 1u << 13; k <= 1u << 23; k++, values++) check_modes(gloss_rec(rgb, (float)k * 0x1p-23f).on, t);
    out[0] = t.checked; out[1] = t.bad; out[2] = t.first_on; out[3] = t.first_modes; out[4] = values;
}
