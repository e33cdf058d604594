// pixel_list_check.cpp -- every refusal of the list form of a render request (mitsuba3dopplertof_amd/csrc/dtof_pixel_list.h: pixel_list_refusal, which check_pixel_list
// of the frame path and the C ABI's entries call before any device call) on the host: one line "name|message" per request, an empty message for one that can run.
// tests/test_adaptive_cpu.py compiles and runs this and holds every message.
#include "dtof_pixel_list.h"
#include <cstdio>

using dtof::PixelListFacts;

static PixelListFacts good() {   // 3 listed pixels of a 8 x 8 crop at 4 spp into the moment film
    PixelListFacts f;
    f.moments = true; f.spp = 4; f.n_pixels = 3; f.crop_pixels = 64;
    return f;
}
static void show(const char *name, const PixelListFacts &f) { printf("%s|%s\n", name, dtof::pixel_list_refusal(f).c_str()); }

int main() {
    PixelListFacts f = good(); show("moments", f);
    f = good(); f.moments = false; f.film64 = true; show("film64", f);
    f = good(); f.film64 = true; show("both films", f);
    f = good(); f.n_pixels = 0; show("empty list", f);
    f = good(); f.n_pixels = 64; show("full list", f);
    f = good(); f.samples_per_pass = 4; show("samples_per_pass == spp", f);
    f = good(); f.samples_per_pass = 0; show("samples_per_pass 0", f);
    f = good(); f.moments = false; f.lane_dump = true; f.dump_begin = 4; f.dump_n = 8; show("dump of whole pixels", f);
    f = good(); f.stripes = true; show("stripes", f);
    f = good(); f.row_range = true; show("row range", f);
    f = good(); f.aov = true; show("aov", f);
    f = good(); f.film32 = true; show("float32 film", f);
    f = good(); f.moments = false; f.film32 = true; show("float32 film alone", f);
    f = good(); f.moments = false; show("no film", f);
    f = good(); f.spp = 0; show("spp 0", f);
    f = good(); f.samples_per_pass = 2; show("samples_per_pass below spp", f);
    f = good(); f.n_pixels = 65; show("more pixels than the crop", f);
    f = good(); f.moments = false; f.lane_dump = true; f.dump_begin = 2; f.dump_n = 8; show("dump begins inside a pixel", f);
    f = good(); f.moments = false; f.lane_dump = true; f.dump_begin = 0; f.dump_n = 6; show("dump ends inside a pixel", f);
    f = good(); f.moments = false; f.lane_dump = true; f.dump_begin = 8; f.dump_n = 8; show("dump beyond the list", f);
    f = good(); f.lane_dump = true; f.dump_n = 6; show("ragged dump with a film", f);
    return 0;
}
