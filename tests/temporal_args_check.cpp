// temporal_args_check.cpp -- every refusal of the temporal stage's two entries (mitsuba3dopplertof_amd/csrc/dtof_temporal_args.h: temporal_check, which both run before
// their first HIP call) on the host: one line "name|message" per argument shape, an empty message for one that can run; then "packed|..." lines with what a good call
// packs.  No pointer is dereferenced: the buffers are addresses inside one large array.  tests/test_temporal_cpu.py compiles and runs this and holds every message.
#include "dtof_temporal_args.h"
#include <cstdio>
#include <limits>
#include <vector>

using dtof::TemporalArgs;
using dtof::TemporalBuffers;

static const int K = 3, W = 6, H = 5;
static std::vector<double> g_arena(14 * 1024);      // 8 KiB per buffer: more than K * W * H * 3 doubles

static const void *slot(int i) { return g_arena.data() + (size_t) i * 1024; }
static TemporalBuffers good() {   // every buffer present, a history included
    return TemporalBuffers { slot(0), slot(1), slot(2), slot(3), slot(4), slot(5), slot(6), slot(7), slot(8), slot(9), slot(10), slot(11), slot(12), slot(13) };
}
static TemporalBuffers first_frame() {
    TemporalBuffers b = good();
    b.h_colour = b.h_variance = b.h_normal = b.h_ids = b.h_length = nullptr;
    return b;
}
struct Call { TemporalBuffers b = good(); int k = K; int32_t w = W, h = H; bool params_null = false; double alpha_min = 0.2, max_length = 32, tau_normal = 0.25; };
static void show(const char *name, const Call &c) {
    TemporalArgs a;
    a.width = -99;
    const std::string err = dtof::temporal_check(c.b, c.k, c.w, c.h, c.params_null, c.alpha_min, c.max_length, c.tau_normal, &a);
    printf("%s|%s\n", name, err.c_str());
    if (!err.empty() && a.width != -99) printf("%s wrote its output although it refused|\n", name);
}
static const void *shifted(const void *p, size_t bytes) { return (const char *) p + bytes; }

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    Call c;
    show("all buffers", c);
    c = Call(); c.b = first_frame(); show("first frame", c);
    c = Call(); c.b = first_frame(); c.b.variance = c.b.o_variance = c.b.normal = c.b.ids = c.b.o_colour_f32 = nullptr; show("colour and flow alone", c);
    c = Call(); c.b.normal = c.b.h_normal = nullptr; c.tau_normal = nan; show("tau_normal unread without normals", c);
    c = Call(); c.k = 1; c.w = 65535; c.h = 65535; c.b = first_frame(); c.b.variance = c.b.o_variance = c.b.normal = c.b.ids = c.b.o_colour_f32 = nullptr;
    c.b.colour = (const void *) 0x1000; c.b.flow = (const void *) 0x1000000000000; c.b.o_colour = (const void *) 0x2000000000000; c.b.o_length = (const void *) 0x3000000000000;
    show("largest extent", c);
    c = Call(); c.alpha_min = 1.0; c.max_length = 1.0; show("alpha_min 1, max_length 1", c);

    c = Call(); c.k = 0; show("0 planes", c);
    c = Call(); c.k = 5; show("5 planes", c);
    c = Call(); c.w = 0; show("width 0", c);
    c = Call(); c.h = 0; show("height 0", c);
    c = Call(); c.w = -3; show("negative width", c);
    c = Call(); c.w = 65536; show("width 65536", c);
    c = Call(); c.h = 65536; show("height 65536", c);
    c = Call(); c.b.colour = nullptr; show("null colour", c);
    c = Call(); c.b.flow = nullptr; show("null flow", c);
    c = Call(); c.b.o_colour = nullptr; show("null o_colour", c);
    c = Call(); c.b.o_length = nullptr; show("null o_length", c);
    c = Call(); c.params_null = true; show("null params", c);
    c = Call(); c.b.h_colour = nullptr; show("history without h_colour", c);
    c = Call(); c.b.h_length = nullptr; show("history without h_length", c);
    c = Call(); c.b.h_variance = nullptr; show("history without h_variance", c);
    c = Call(); c.b.h_normal = nullptr; show("history without h_normal", c);
    c = Call(); c.b.h_ids = nullptr; show("history without h_ids", c);
    c = Call(); c.b = first_frame(); c.b.h_length = slot(9); show("h_length alone", c);
    c = Call(); c.b.variance = c.b.o_variance = nullptr; show("h_variance without variance", c);
    c = Call(); c.b.normal = nullptr; show("h_normal without normal", c);
    c = Call(); c.b.ids = nullptr; show("h_ids without ids", c);
    c = Call(); c.b.variance = c.b.h_variance = nullptr; show("o_variance without variance", c);
    c = Call(); c.b.o_variance = nullptr; show("variance without o_variance", c);
    c = Call(); c.b.colour = shifted(c.b.colour, 2); show("misaligned colour", c);
    c = Call(); c.b.variance = shifted(c.b.variance, 4); show("misaligned variance", c);
    c = Call(); c.b.h_colour = shifted(c.b.h_colour, 4); show("misaligned h_colour", c);
    c = Call(); c.b.o_colour = shifted(c.b.o_colour, 4); show("misaligned o_colour", c);
    c = Call(); c.b.o_length = shifted(c.b.o_length, 1); show("misaligned o_length", c);
    c = Call(); c.b.o_colour_f32 = shifted(c.b.o_colour_f32, 2); show("misaligned o_colour_f32", c);
    c = Call(); c.b.o_colour = c.b.h_colour; show("o_colour is h_colour", c);
    c = Call(); c.b.o_length = c.b.h_length; show("o_length is h_length", c);
    c = Call(); c.b.o_variance = c.b.variance; show("o_variance is variance", c);
    c = Call(); c.b.o_colour_f32 = c.b.colour; show("o_colour_f32 is colour", c);
    c = Call(); c.b.o_length = shifted(c.b.flow, (size_t) W * H * 8 - 4); show("o_length begins in the last word of flow", c);
    c = Call(); c.b.o_length = shifted(c.b.flow, (size_t) W * H * 8); show("o_length begins behind flow", c);
    c = Call(); c.b.o_variance = shifted(c.b.o_colour, (size_t) K * W * H * 24 - 8); show("o_variance begins in the last word of o_colour", c);
    c = Call(); c.b.o_colour_f32 = c.b.o_length; show("o_colour_f32 is o_length", c);
    c = Call(); c.alpha_min = 0.0; show("alpha_min 0", c);
    c = Call(); c.alpha_min = -0.5; show("alpha_min negative", c);
    c = Call(); c.alpha_min = 1.5; show("alpha_min above 1", c);
    c = Call(); c.alpha_min = nan; show("alpha_min nan", c);
    c = Call(); c.max_length = 0.5; show("max_length below 1", c);
    c = Call(); c.max_length = inf; show("max_length inf", c);
    c = Call(); c.max_length = nan; show("max_length nan", c);
    c = Call(); c.tau_normal = 0.0; show("tau_normal 0", c);
    c = Call(); c.tau_normal = -1.0; show("tau_normal negative", c);
    c = Call(); c.tau_normal = inf; show("tau_normal inf", c);
    c = Call(); c.tau_normal = nan; show("tau_normal nan", c);
    c = Call(); c.tau_normal = 1e-200; show("tau_normal squared underflows", c);
    c = Call(); c.tau_normal = 1e200; show("tau_normal squared overflows", c);

    TemporalArgs a;
    c = Call(); c.tau_normal = 0.3;
    if (!dtof::temporal_check(c.b, c.k, c.w, c.h, false, c.alpha_min, c.max_length, c.tau_normal, &a).empty()) return 1;
    printf("packed|%d %d %d %d %d %d %d %.17g %.17g %.17g\n", a.width, a.height, a.n_planes, a.has_variance, a.has_normal, a.has_ids, a.has_history, a.alpha_min,
           a.max_length, a.tau_normal2);
    c.b = first_frame(); c.b.normal = nullptr; c.b.ids = nullptr;
    if (!dtof::temporal_check(c.b, c.k, c.w, c.h, false, c.alpha_min, c.max_length, c.tau_normal, &a).empty()) return 1;
    printf("packed first|%d %d %d %d %d %d %d %.17g %.17g %.17g\n", a.width, a.height, a.n_planes, a.has_variance, a.has_normal, a.has_ids, a.has_history, a.alpha_min,
           a.max_length, a.tau_normal2);
    return 0;
}
