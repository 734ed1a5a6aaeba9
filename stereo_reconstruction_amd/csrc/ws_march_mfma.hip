// ws_march_mfma.hip -- the SSD search on the int8 matrix cores: instantiations, the rule that selects it, its tiling
// and its launcher.  The kernel and the formulation: ws_march_mfma.h.  Everything it does not take stays on the stencil
// kernel (ws_march.hip): SAD, the right view, centred windows, ranges beyond one d-group pass, cost planes, forced tunings.
#include "ws_march_mfma.h"
#include "ws_march_plan.h"

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

// The smallest search the kernel is taken for.  A workgroup holds a CU to itself (134 KB of LDS), so a small search
// leaves it strips of a few rows whose warm-up and stage steps dominate; below these sizes the stencil kernel keeps the
// search (profiles/mfma_ssd/README.md: the ladder of sizes).
constexpr int kMfmaMinCols = 384, kMfmaMinRows = 192;

bool march_mfma_plan(const Canon &c, int num_cus, MarchLaunch *out)
{
    const int knob = march_knobs().mfma;
    if (knob == 0 || march_knobs().stencil_forced) return false;
    const int dcount = c.d_hi - c.d_lo + 1, out_w = c.ox1 - c.ox0, out_h = c.oy1 - c.oy0;
    const MfmaEntry *e = find_mfma(c);
    if (!c.ssd || c.mirror || !c.prefer_large || !e) return false;
    if (dcount < 1 || dcount > 32 * (kMfmaVTiles - 1) || out_w < 1 || out_h < 1 || num_cus < 1) return false;
    if (knob != 1 && (out_w < kMfmaMinCols || out_h < kMfmaMinRows)) return false;
    MarchLaunch m{};
    m.mfma = 1;
    m.fn = e->fn;
    m.name = e->name;
    m.centred = out->centred; // (the packed planes beside the kernel stay what the stencil plan packs)
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
    // One workgroup per CU (its accumulators fill the register file): a round of strips is num_cus workgroups.
    const int forced_rows = march_knobs().mfma_strip_rows;
    const int strips = forced_rows > 0 ? ceil_div(out_h, forced_rows) : best_strips(kMfmaStrips, out_h, m.tiles, c.wh, num_cus).strips;
    m.strip_rows = ceil_div(out_h, strips);
    m.strips = ceil_div(out_h, m.strip_rows);
    // the packed key's ranges are derived for strips of up to kMfmaMaxSteps rows entered (ws_march_mfma.h)
    if (m.strip_rows + c.wh - 1 > kMfmaMaxSteps) return false;
    *out = m;
    return true;
}

hipError_t launch_march_mfma(const Canon &c, const MarchLaunch &m, const MarchIo &io, hipStream_t s)
{
    if (!m.mfma || !m.fn || m.tile_cols != 32 * kMfmaXWaves || m.threads != 64 * kMfmaWaves) return hipErrorInvalidValue;
    const MarchArgs g = march_args(c, m, io);
    if (m.lds_bytes > 48 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(m.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)m.lds_bytes);
        if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(m.fn, dim3(round_up(m.tiles * m.strips, 8)), dim3(m.threads), m.lds_bytes, s, g);
    return hipGetLastError();
}

} // namespace wsamd
