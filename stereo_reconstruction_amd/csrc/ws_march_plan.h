// ws_march_plan.h -- what the two marching translation units (ws_march.hip: planner and launcher; ws_march_mfma.hip:
// the matrix-core kernel's rule and launcher) share on the host and nobody else sees: the development knobs, the strip
// model, the kernels' argument block and the matrix kernel's entry points.
#pragma once
#include "ws_march_kernel.h"

namespace wsamd {

// Every development knob of the marching path, read from the environment once, on first use (march_knobs).
struct MarchKnobs {
    int nd = 0;                  // WS_MARCH_ND: 8 or 4 disparities per thread, whatever the model says (0 = the model)
    bool halo_off = false;       // WS_MARCH_HALO: 0 = never the halo-exchange kernels
    bool halo_ssd_off = false;   // WS_MARCH_HALO_SSD: 0 = not for SSD
    int slots = 0;               // WS_PLAN_SLOTS: workgroups per CU the strip model plans with (> 0)
    int threads = 0;             // WS_PLAN_THREADS: workgroup size (>= 64), as ws_set_tuning's threads
    int max_chunks = 0;          // WS_MAX_CHUNKS: d-chunks per tile and pass at most, within [8, kMaxT / 4] (else ignored)
    int stage_wave = -1;         // WS_STAGE_WAVE / WS_FLUSH_WAVE: the first wave that unpacks / that flushes; -1 = default
    int flush_wave = -1;
    int stage_agap = 0;          // WS_STAGE_AGAP: image A's stage roles this many places behind image B's
    int mfma = -1;               // WS_MARCH_MFMA: 0 = never the matrix-core SSD kernel, 1 = wherever it can run (whatever the
                                 // search's size)
    int mfma_strip_rows = 0;     // WS_MFMA_STRIP_ROWS: rows per strip of the matrix-core kernel (> 0), whatever the strip
                                 // model says: a development knob (one long strip in a small image)
    bool stencil_forced = false; // WS_PLAN_SLOTS, WS_PLAN_THREADS, WS_MAX_CHUNKS or WS_MARCH_ND is set (to anything): the
                                 // stencil kernel's knobs keep meaning the stencil kernel
};
const MarchKnobs &march_knobs();

// The strip model.  The chip works through ceil(workgroups / capacity) rounds of strips, capacity = CUs x workgroups
// per CU; a strip of R rows costs R row steps, `warm` of a step for each of the window's wh - 1 warm-up rows and
// `prologue` steps for the stages that run ahead of the first row.
struct StripModel { double warm, prologue; };
// the stencil kernel: the warm-up rows only add, the prologue is worth ~3 rows (config 3's own sweep,
// profiles/r01/sweep_tiles_config3.csv, has its minimum where this puts it)
constexpr StripModel kStencilStrips{0.5, 3.0};
// the matrix kernel: a warm-up row is one MFMA per tile instead of two and no keys, ~2 steps for the three steps of the
// stages alone (profiles/mfma_ssd/README.md)
constexpr StripModel kMfmaStrips{0.35, 2.0};
inline double strip_cost(StripModel k, int wgs_per_row, int strips, int rows, int wh, int capacity)
{
    return ceil_div(wgs_per_row * strips, capacity) * (rows + k.warm * (wh - 1) + k.prologue);
}
struct StripChoice { int strips; double cost; };
// the strip count with the cheapest total among all that cut out_h rows differently; the first minimum wins
inline StripChoice best_strips(StripModel k, int out_h, int wgs_per_row, int wh, int capacity)
{
    StripChoice best{1, 0.0};
    for (int sc = 1; sc <= out_h; ++sc) {
        const int rows = ceil_div(out_h, sc);
        if (ceil_div(out_h, rows) != sc) continue; // (the same strips as a smaller count already seen)
        const double cost = strip_cost(k, wgs_per_row, sc, rows, wh, capacity);
        if (sc == 1 || cost < best.cost) best = {sc, cost};
    }
    return best;
}

// The argument block of either kernel's first (or only) launch.  The matrix kernel (m.mfma) counts its tie tags from d_hi
// and has one pass, no cost plane, no global tie tags and no stage knobs: those fields keep their defaults.
inline MarchArgs march_args(const Canon &c, const MarchLaunch &m, const MarchIo &io)
{
    MarchArgs g{};
    g.st.img_a = io.img_a;
    g.st.stride_a = io.stride_a;
    g.st.img_b = io.img_b;
    g.st.stride_b = io.stride_b;
    g.st.wa = c.wa;
    g.st.wb = c.wb;
    g.st.nxr = m.nxr;
    g.st.nch = m.nch;
    g.st.wx0 = c.wx0;
    g.st.boff = c.boff;
    g.st.d_first = c.d_lo;
    g.st.mirror = c.mirror;
    g.st.b_lo = c.b_lo;
    g.st.b_hi = c.b_hi;
    g.out = io.out;
    g.out16 = io.out16;
    g.out_pitch = io.out_pitch;
    g.border = io.border;
    g.out_w = io.out_w;
    g.out_h = io.out_h;
    g.wy0 = c.wy0;
    g.d_lo = c.d_lo;
    g.d_hi = c.d_hi;
    g.d_top = m.mfma ? c.d_hi : c.d_lo + m.passes * m.nch * m.nd_per_thread - 1;
    g.ox0 = c.ox0;
    g.ox1 = c.ox1;
    g.oy0 = c.oy0;
    g.oy1 = c.oy1;
    g.strip_rows = m.strip_rows;
    g.tiles = m.tiles;
    g.strips = m.strips;
    g.tile_stride = m.tile_cols;
    g.prefer_large = c.prefer_large;
    g.fallback_neg = c.fallback_neg;
    g.tune_prod_wave = g.tune_flush_wave = -1;
    if (m.mfma) return g;
    const MarchKnobs &k = march_knobs();
    g.keys = io.keys;
    g.keys_pitch = io.keys_pitch;
    g.tag_bits = m.tag_bits;
    g.cost_out = io.cost_out;
    g.cost_pitch = io.cost_pitch;
    g.tune_prod_wave = k.stage_wave;
    g.tune_flush_wave = k.flush_wave;
    g.tune_a_gap = k.stage_agap;
    return g;
}

// The SSD search on the int8 matrix cores (ws_march_mfma.hip): plain bytes, left view, one d-group pass of up to 256
// candidates, a window it is instantiated for, and a search big enough to fill the chip with its 128-column tiles.
// march_mfma_plan replaces the stencil plan in *out if the search is one of those (march_plan asks it when nothing is
// tuned by hand); it keeps that plan's `centred`.
bool march_mfma_plan(const Canon &c, int num_cus, MarchLaunch *out);
hipError_t launch_march_mfma(const Canon &c, const MarchLaunch &m, const MarchIo &io, hipStream_t s);

} // namespace wsamd
