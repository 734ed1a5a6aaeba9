// ws_march_mfma.hip -- the SSD search on the int8 matrix cores: instantiations, the rule that selects it, its tiling
// and its launcher.  The kernel and the formulation: ws_march_mfma.h.  Everything it does not take stays on the stencil
// kernel (ws_march.hip): SAD, the right view, centred windows, ranges beyond one d-group pass, cost planes, forced tunings.
#include "ws_march_mfma.h"

#include <stdlib.h>

namespace wsamd {

struct MfmaEntry {
    int ww, wh;
    MarchFn fn;
    const char *name;
};
static const MfmaEntry kMfmaTable[] = {
    {7, 7, ws_march_mfma_kernel<7, 7>, "ws_march_kernel<ssd,7x7,mfma>"},
};

static const MfmaEntry *find_mfma(const Canon &c)
{
    for (const MfmaEntry &e : kMfmaTable)
        if (e.ww == c.ww && e.wh == c.wh) return &e;
    return nullptr;
}

// WS_MARCH_MFMA (development knob, read once): 0 = never, 1 = wherever the kernel can run (whatever the search's size)
static int mfma_knob()
{
    static const int v = [] {
        const char *e = getenv("WS_MARCH_MFMA");
        return e ? atoi(e) : -1;
    }();
    return v;
}

// The smallest search the kernel is taken for.  A workgroup holds a CU to itself (134 KB of LDS), so a small search
// leaves it strips of a few rows whose warm-up and stage steps dominate; below these sizes the stencil kernel keeps the
// search (profiles/mfma_ssd/README.md: the ladder of sizes).
constexpr int kMfmaMinCols = 384, kMfmaMinRows = 192;

bool march_mfma_plan(const Canon &c, int num_cus, MarchLaunch *out)
{
    const int knob = mfma_knob();
    if (knob == 0) return false;
    // the stencil kernel's development knobs keep meaning the stencil kernel
    static const bool stencil_forced = [] {
        for (const char *n : {"WS_PLAN_SLOTS", "WS_PLAN_THREADS", "WS_MAX_CHUNKS", "WS_MARCH_ND"})
            if (getenv(n)) return true;
        return false;
    }();
    if (stencil_forced) return false;
    const int dcount = c.d_hi - c.d_lo + 1, out_w = c.ox1 - c.ox0, out_h = c.oy1 - c.oy0;
    if (!c.ssd || c.mirror || !c.prefer_large || !find_mfma(c)) return false;
    if (dcount < 1 || dcount > 32 * (kMfmaVTiles - 1) || out_w < 1 || out_h < 1 || num_cus < 1) return false;
    if (knob != 1 && (out_w < kMfmaMinCols || out_h < kMfmaMinRows)) return false;
    MarchLaunch m{};
    m.mfma = 1;
    m.x_per_thread = 8;
    m.nd_per_thread = 8;
    m.nxr = 4 * kMfmaXWaves;       // a tile's 128 columns, in runs of 8
    m.nch = 4 * (kMfmaVTiles - 1); // ... and its 256 candidates, in chunks of 8
    m.passes = 1;
    m.threads = m.max_threads = 64 * kMfmaWaves;
    m.halo = 0;
    m.tile_cols = 32 * kMfmaXWaves;
    m.tiles = ceil_div(out_w, m.tile_cols);
    m.lds_bytes = (size_t)mfma_lds_layout(c.ww, c.wh).bytes;
    // One workgroup per CU (its accumulators fill the register file).  A strip of R rows costs about R row steps, a
    // third of a step for each of the wh - 1 warm-up rows (one MFMA per tile instead of two, no keys) and ~2 for the
    // three steps of the stages alone; the chip works through ceil(workgroups / CUs) rounds of them.
    int strips = 1;
    double best_cost = 0.0;
    for (int sc = 1; sc <= out_h; ++sc) {
        const int rows = ceil_div(out_h, sc), st = ceil_div(out_h, rows);
        if (st != sc) continue;
        const double cost = ceil_div(m.tiles * st, num_cus) * (rows + 0.35 * (c.wh - 1) + 2.0);
        if (sc == 1 || cost < best_cost) { best_cost = cost; strips = sc; }
    }
    m.strip_rows = ceil_div(out_h, strips);
    m.strips = ceil_div(out_h, m.strip_rows);
    *out = m;
    return true;
}

const char *march_mfma_kernel_name(const Canon &c)
{
    const MfmaEntry *e = find_mfma(c);
    return e ? e->name : "";
}

hipError_t launch_march_mfma(const Canon &c, const MarchLaunch &m, const uint8_t *img_a, int stride_a, const uint8_t *img_b, int stride_b,
                             float *out, int16_t *out16, int out_pitch, int border, int out_w, int out_h, hipStream_t s)
{
    const MfmaEntry *e = find_mfma(c);
    if (!e || !m.mfma || m.tile_cols != 32 * kMfmaXWaves || m.threads != 64 * kMfmaWaves) return hipErrorInvalidValue;
    MarchArgs g{};
    g.st.img_a = img_a;
    g.st.stride_a = stride_a;
    g.st.img_b = img_b;
    g.st.stride_b = stride_b;
    g.st.wa = c.wa;
    g.st.wb = c.wb;
    g.st.nxr = m.nxr;
    g.st.nch = m.nch;
    g.st.wx0 = c.wx0;
    g.st.boff = c.boff;
    g.st.d_first = c.d_lo;
    g.st.mirror = 0;
    g.st.b_lo = c.b_lo;
    g.st.b_hi = c.b_hi;
    g.out = out;
    g.out16 = out16;
    g.out_pitch = out_pitch;
    g.border = border;
    g.out_w = out_w;
    g.out_h = out_h;
    g.wy0 = c.wy0;
    g.d_lo = c.d_lo;
    g.d_hi = c.d_hi;
    g.d_top = c.d_hi;
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
    if (m.lds_bytes > 48 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(e->fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)m.lds_bytes);
        if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(e->fn, dim3(round_up(m.tiles * m.strips, 8)), dim3(m.threads), m.lds_bytes, s, g);
    return hipGetLastError();
}

} // namespace wsamd
