// ws_search.cpp -- argument checks that stand in for the reference's cv::Exception paths, reduction of the three
// reference methods to the canonical search (ws_kernels.h), and the launches of one search (ws_search.h).
#include "ws_search.h"
#include "ws_ct.h"
#include "ws_staging.h"

#include <string.h>

#include <algorithm>

namespace wsamd {

namespace {

// What a canonical search leaves for the passes after it (smoothFactor).
struct SearchResult {
    bool planes = false; // the marching kernel ran and packed the dword planes (canon, plan, pa and pb are read only then)
    Canon canon{};
    MarchLaunch plan{};
    Plane pa{}, pb{};
    int32_t *cost = nullptr;           // the winners' costs (pitch canon.wa), or null
    const int32_t *bs_plane = nullptr; // varBlock: the windows ws_varblock_kernel chose (pitch (R->width + 63) & ~63)
};

// the brute-force kernels' view of a search (ws_kernels.h)
GenericArgs generic_args(const ws_params *p, const ws_image *L, const ws_image *R, float *out, int out_stride)
{
    GenericArgs ga{};
    ga.L = L->data; ga.R = R->data;
    ga.w1 = L->width; ga.h1 = L->height; ga.s1 = L->stride;
    ga.w2 = R->width; ga.h2 = R->height; ga.s2 = R->stride;
    ga.view = p->view; ga.ssd = p->cost == WS_COST_SSD;
    ga.block_size = p->block_size; ga.min_d = p->min_disparity; ga.max_d = p->max_disparity;
    ga.linear_range = p->linear_range;
    ga.out = out; ga.out_pitch = out_stride;
    return ga;
}

// the brute-force kernels leave the marching kernel's interior (in original coordinates) alone
void skip_interior(const Canon &c, GenericArgs *ga)
{
    ga->skip_x0 = c.mirror ? c.wa - c.ox1 : c.ox0;
    ga->skip_x1 = c.mirror ? c.wa - c.ox0 : c.ox1;
    ga->skip_y0 = c.oy0; ga->skip_y1 = c.oy1;
}

// One search with smoothFactor 1: the marching kernel where a marching region exists, and the kernels for the rest.
// keep_cost: also leave the winners' costs (the right view's smoothFactor passes); pack_planes: also pack the dword
// planes (the left view's smoothFactor pass reads them).
int run_canonical(Searcher &S, std::string *err, const ws_params *p, const ws_image *L, const ws_image *R, float *out,
                  int out_stride, int16_t *out16, bool keep_cost, bool pack_planes, hipStream_t s, SearchResult *res)
{
    const int ow = p->view == WS_VIEW_LEFT ? L->width : R->width;
    if (out_stride < ow) return fail(err, WS_ERR_ARG, "out_stride %d < width %d", out_stride, ow);

    GenericArgs ga = generic_args(p, L, R, out, out_stride);
    ga.out16 = out16;

    *res = SearchResult{};
    if (p->view == WS_VIEW_RIGHT) S.var_block_ran = false;
    if (p->view == WS_VIEW_RIGHT && p->var_block) {
        // the ordinary search first; then one wave per pixel decides the window (ws_varblock_kernel)
        // and searches again only where it grew
        ws_params q = *p;
        q.var_block = 0;
        q.subpixel = 0;
        int rc = run_canonical(S, err, &q, L, R, out, out_stride, out16, keep_cost, pack_planes, s, res);
        if (rc != WS_OK) return rc;
        const int bs_pitch = (R->width + 63) & ~63;
        if ((rc = ensure(err, S.bs_plane, (size_t)bs_pitch * R->height * sizeof(int32_t))) != WS_OK) return rc;
        if ((rc = ensure(err, S.max_block, 64)) != WS_OK) return rc;
        WS_HIP(err, launch_varblock(ga, p->thres, static_cast<int32_t *>(S.bs_plane.p), bs_pitch,
                                    static_cast<int *>(S.max_block.p), s));
        res->bs_plane = static_cast<const int32_t *>(S.bs_plane.p);
        S.launched("ws_varblock_kernel", 256, (int)(((long long)R->width * R->height + 3) / 4), 0);
        S.var_block_ran = true;
        return WS_OK;
    }
    Canon c{};
    MarchLaunch m{};
    bool march = make_canon(p, L, R, &c);
    if (march) {
        const Searcher::CachedPlan &plan = S.plan_for(c);
        m = plan.launch;
        march = plan.ok;
    }
    // Dword planes of both images: only for the kernels BESIDE the marching kernel that still read them -- the right
    // view's border ring, the sub-pixel refine, the smoothFactor passes.  The marching kernel reads the caller's bytes.
    const bool planes = march && (p->view == WS_VIEW_RIGHT || p->subpixel || pack_planes);
    if (march) {
        int rc;
        const ws_image *ia = p->view == WS_VIEW_LEFT ? L : R;
        const ws_image *ib = p->view == WS_VIEW_LEFT ? R : L;
        skip_interior(c, &ga);
        if (planes) {
            Plane &pa = res->pa, &pb = res->pb;
            march_plane_geometry(c, m, &pa, &pb);
            if ((rc = ensure(err, S.plane_a, (size_t)pa.pitch * c.ha * 4)) != WS_OK) return rc;
            if ((rc = ensure(err, S.plane_b, (size_t)pb.pitch * c.hb * 4)) != WS_OK) return rc;
            pa.data = static_cast<uint32_t *>(S.plane_a.p);
            pb.data = static_cast<uint32_t *>(S.plane_b.p);
            WS_HIP(err, launch_pack(c, m, ia->data, ia->stride, pa, ib->data, ib->stride, pb, s));
        }
        if (S.profiling) WS_HIP(err, hipEventRecord(S.evk0, s));
        const int keys_pitch = (c.wa + 15) & ~15;
        if (m.passes > 1 && (rc = ensure(err, S.keys, (size_t)keys_pitch * c.ha * 8)) != WS_OK) return rc;
        if (keep_cost && m.fn_cost) {
            if ((rc = ensure(err, S.cost, (size_t)c.wa * c.ha * 4)) != WS_OK) return rc;
            res->cost = static_cast<int32_t *>(S.cost.p);
        }
        // left view: the marching kernel also writes the zeros outside its interior (BlockSearch.cpp:33,36,38); the
        // right view's ring runs on the packed planes after it
        MarchIo io{};
        io.img_a = ia->data; io.stride_a = ia->stride; io.img_b = ib->data; io.stride_b = ib->stride;
        io.out = out; io.out16 = out16; io.out_pitch = out_stride;
        io.border = p->view == WS_VIEW_LEFT; io.out_w = L->width; io.out_h = L->height;
        io.keys = S.keys.p; io.keys_pitch = keys_pitch;
        io.cost_out = res->cost; io.cost_pitch = c.wa;
        WS_HIP(err, launch_march(c, m, io, s));
        if (S.profiling) {
            WS_HIP(err, hipEventRecord(S.evk1, s));
            S.kernel_timed = true;
        }
        S.launched(m.name, m.threads, m.tiles * m.strips, (int)m.lds_bytes);
    } else {
        // (launch_linear hands ranges beyond kLinearMaxRange to the brute-force kernel: name the one that runs)
        S.launched(p->view == WS_VIEW_LINEAR && p->linear_range <= kLinearMaxRange ? "ws_linear_kernel" : "ws_generic_kernel", 256,
                   ((ow + 255) / 256) * (p->view == WS_VIEW_LEFT ? L->height : R->height), 0);
    }
    // everything the marching kernel does not own: border ring, rows past min(h1,h2), or all of it
    if (march && p->view == WS_VIEW_RIGHT)
        WS_HIP(err, launch_ring(c, m, res->pa, res->pb, ga, out, out_stride, res->cost, c.wa, s));
    else if (!march && p->view == WS_VIEW_LINEAR)
        WS_HIP(err, launch_linear(ga, s));
    else if (!march)
        WS_HIP(err, launch_generic(ga, s));
    res->planes = planes;
    res->canon = c;
    res->plan = m;
    if (p->subpixel) {
        if (march) WS_HIP(err, launch_refine_planes(c, m, res->pa, res->pb, out, out_stride, s));
        WS_HIP(err, launch_refine(ga, s)); // the pixels outside the marching interior (all of them without it)
    }
    return WS_OK;
}

// A census-transform cost (smoothFactor 1, no varBlock: check_params): both images' descriptors into the Searcher's
// planes, then the match kernel, which writes the whole map itself -- winners, fallbacks, zeros and the parabola.
int run_census(Searcher &S, std::string *err, const ws_params *p, const ws_image *L, const ws_image *R, float *out, int out_stride,
               hipStream_t s)
{
    int ow, oh;
    map_dims(p, L, R, &ow, &oh);
    if (out_stride < ow) return fail(err, WS_ERR_ARG, "out_stride %d < width %d", out_stride, ow);
    const size_t esz = census_plane_elem(p->cost);
    int rc;
    if ((rc = ensure(err, S.ct_left, (size_t)L->width * L->height * esz)) != WS_OK) return rc;
    if ((rc = ensure(err, S.ct_right, (size_t)R->width * R->height * esz)) != WS_OK) return rc;
    WS_HIP(err, launch_census_transform(L->data, L->width, L->height, L->stride, p->cost, S.ct_left.p, L->width, false, s));
    WS_HIP(err, launch_census_transform(R->data, R->width, R->height, R->stride, p->cost, S.ct_right.p, R->width, false, s));
    CtMatchArgs a = census_match_args(p, L, R, S.ct_left.p, S.ct_right.p);
    a.out = out;
    a.out_pitch = out_stride;
    if (S.profiling) WS_HIP(err, hipEventRecord(S.evk0, s));
    WS_HIP(err, launch_census_match(a, false, s));
    if (S.profiling) {
        WS_HIP(err, hipEventRecord(S.evk1, s));
        S.kernel_timed = true;
    }
    if (p->view == WS_VIEW_RIGHT) S.var_block_ran = false;
    S.launched(kCtMatchKernel, kCtThreads, (int)census_match_workgroups(ow, oh), kCtLdsWta);
    return WS_OK;
}

// smoothFactor: the data-parallel search (smoothFactor 1) first, then the smoothFactor passes on its map.  For the right
// view and LinearSearch the factor can only reach d = 0 beside a zero-valued neighbour (see ws_smooth.hip), and only
// when d = 0 is a candidate at all.
int search_on(Searcher &S, std::string *err, const ws_params *p, const ws_image *L, const ws_image *R, float *out,
              int out_stride, int16_t *out16, unsigned int *status, hipStream_t s)
{
    ws_params q = *p;
    SearchResult r;
    if (q.view == WS_VIEW_LINEAR) q.min_disparity = 0;
    if (q.view != WS_VIEW_LINEAR && is_census(q.cost)) return run_census(S, err, &q, L, R, out, out_stride, s);
    const bool left = q.view == WS_VIEW_LEFT;
    if (q.smooth_factor == 1.0 || (!left && q.min_disparity != 0))
        return run_canonical(S, err, &q, L, R, out, out_stride, out16, false, false, s, &r);
    GenericArgs ga = generic_args(p, L, R, out, out_stride);
    ga.min_d = 0;
    int rc;
    if (left) { // d1 from the data-parallel search; the raster-order pass does the rest
        q.smooth_factor = 1.0;
        if ((rc = run_canonical(S, err, &q, L, R, out, out_stride, nullptr, false, true, s, &r)) != WS_OK) return rc;
        // per pixel the best candidate's cost (0 <= s <= 1) or the three best candidates
        if ((rc = ensure(err, S.top3, smooth_left_top_bytes(L->width, L->height, p->smooth_factor))) != WS_OK) return rc;
        WS_HIP(err, launch_smooth_left(ga, p->smooth_factor, static_cast<uint32_t *>(S.top3.p), r.planes ? &r.canon : nullptr,
                                       &r.plan, r.pa, r.pb, status, s));
        return WS_OK;
    }
    q.min_disparity = 1; // the data-parallel part: best candidate among d >= 1
    q.subpixel = 0;
    // (the right view without varBlock keeps its marching kernel's planes and cost plane for the passes)
    if ((rc = run_canonical(S, err, &q, L, R, out, out_stride, nullptr, p->view == WS_VIEW_RIGHT && !p->var_block, false, s, &r)) != WS_OK)
        return rc;
    const int sel_pitch = (R->width + 63) & ~63;
    if ((rc = ensure(err, S.sel, (size_t)sel_pitch * (smooth_sel_rows(R->height) + 64))) != WS_OK) return rc;
    if (r.bs_plane) { // the windows ws_varblock_kernel chose
        ga.bs_plane = r.bs_plane;
        ga.bs_pitch = (R->width + 63) & ~63;
    }
    if ((rc = ensure(err, S.sel_planes, smooth_planes_bytes(R->width, R->height))) != WS_OK) return rc;
    const bool on_planes = r.planes && r.cost;
    if (on_planes) skip_interior(r.canon, &ga);
    WS_HIP(err, launch_smooth(ga, p->smooth_factor, static_cast<uint8_t *>(S.sel.p), sel_pitch,
                              static_cast<unsigned long long *>(S.sel_planes.p), on_planes ? &r.canon : nullptr, &r.plan, r.pa, r.pb,
                              on_planes ? r.cost : nullptr, on_planes ? r.canon.wa : 0, s));
    return WS_OK;
}

} // namespace

const Searcher::CachedPlan &Searcher::plan_for(const Canon &c)
{
    for (const CachedPlan &e : plans)
        if (e.valid && !memcmp(&e.canon, &c, sizeof c) && !memcmp(e.tune, tune, sizeof tune)) return e;
    CachedPlan &e = plans[plan_next];
    plan_next = (plan_next + 1) % (int)(sizeof plans / sizeof plans[0]);
    e.launch = MarchLaunch{};
    e.ok = march_plan(c, num_cus, tune[0], tune[1], tune[2], &e.launch);
    e.canon = c;
    memcpy(e.tune, tune, sizeof tune);
    e.valid = true;
    return e;
}

int check_params(std::string *err, const ws_params *p, const ws_image *L, const ws_image *R)
{
    if (!p || !image_ok(L) || !image_ok(R)) return fail(err, WS_ERR_ARG, "null or malformed image / params");
    if (p->view != WS_VIEW_LEFT && p->view != WS_VIEW_RIGHT && p->view != WS_VIEW_LINEAR)
        return fail(err, WS_ERR_ARG, "unknown view %d", p->view);
    if (p->cost != WS_COST_SSD && p->cost != WS_COST_SAD && !is_census(p->cost)) return fail(err, WS_ERR_ARG, "unknown cost %d", p->cost);
    if (p->view != WS_VIEW_LINEAR && (p->block_size < 1 || p->block_size > 63))
        return fail(err, WS_ERR_ARG, "blockSize %d outside [1,63]", p->block_size);
    if (p->view == WS_VIEW_LINEAR && p->linear_range < 1) return fail(err, WS_ERR_ARG, "linear_range < 1");
    if (!(p->smooth_factor == p->smooth_factor)) return fail(err, WS_ERR_ARG, "smoothFactor is NaN");
    if (p->var_block && p->view == WS_VIEW_RIGHT && p->subpixel)
        return fail(err, WS_ERR_UNSUPPORTED, "sub-pixel refinement together with varBlock");
    if (p->var_block && p->view == WS_VIEW_RIGHT && !(p->thres == p->thres))
        return fail(err, WS_ERR_ARG, "thres is NaN");
    if (p->subpixel && p->view == WS_VIEW_LINEAR) return fail(err, WS_ERR_UNSUPPORTED, "sub-pixel on LinearSearch");
    if (p->subpixel && p->smooth_factor != 1.0) return fail(err, WS_ERR_UNSUPPORTED, "sub-pixel refinement together with smoothFactor != 1");
    // (LinearSearch ignores the cost; the refusals the reference's own rules make come first and keep their codes)
    const bool census = is_census(p->cost) && p->view != WS_VIEW_LINEAR;
    const int h1 = L->height, w1 = L->width, h2 = R->height;
    const int height = std::min(h1, h2);
    const int half = (p->block_size - 1) / 2;
    if (p->view == WS_VIEW_LEFT) {
        // Rect(x-half, y-half, bs, bs) leaves the image for even bs (BlockSearch.cpp:46-49)
        if ((p->block_size & 1) == 0 && height - 2 * half > 0 && w1 - 2 * half > 0)
            return fail(err, WS_ERR_GEOMETRY, "even blockSize %d: the reference throws cv::Exception", p->block_size);
    } else if (p->view == WS_VIEW_RIGHT && p->max_disparity > p->min_disparity) {
        if (p->min_disparity < 0)
            return fail(err, WS_ERR_GEOMETRY, "minDisparity < 0: left ROI starts before column 0 (BlockSearch.cpp:151)");
        // leftImage_(Rect(.., y-up, .., up+down)) needs y + down <= h1 (BlockSearch.cpp:151-154)
        for (int y = std::max(0, height - half - 1); y < height; ++y) { // (only the last rows can overrun)
            const int down = std::min(h2 - y - 1, half);
            if (y + down > h1)
                return fail(err, WS_ERR_GEOMETRY, "left image too short for the right view window at row %d", y);
        }
        // varBlock grows windows by data: with a right image taller than the left one a grown window near
        // row h1 needs left-image rows >= h1 and the reference throws (BlockSearch.cpp:151-154) -- but only
        // if such a pixel happens to grow.  Defined here: rejected up front, whatever the data.
        if (p->var_block && h2 > h1)
            return fail(err, WS_ERR_GEOMETRY, "varBlock with a right image taller than the left one: a grown window "
                                              "would leave the left image (BlockSearch.cpp:151-154)");
    }
    if (census && p->smooth_factor != 1.0) return fail(err, WS_ERR_UNSUPPORTED, "a census cost together with smoothFactor != 1");
    if (census && p->view == WS_VIEW_RIGHT && p->var_block) return fail(err, WS_ERR_UNSUPPORTED, "a census cost together with varBlock");
    return WS_OK;
}

int check_out(std::string *err, const ws_params *p, const ws_image *L, const ws_image *R, const void *out, int out_stride,
              int out_dtype, int *ow, int *oh)
{
    map_dims(p, L, R, ow, oh);
    if (!out || (out_dtype != WS_OUT_F32 && out_dtype != WS_OUT_F64)) return fail(err, WS_ERR_ARG, "bad output");
    if (out_stride < *ow) return fail(err, WS_ERR_ARG, "out_stride %d < width %d", out_stride, *ow);
    return WS_OK;
}

bool make_canon(const ws_params *p, const ws_image *L, const ws_image *R, Canon *c)
{
    const int h1 = L->height, w1 = L->width, h2 = R->height, w2 = R->width;
    const int height = std::min(h1, h2);
    const int half = (p->block_size - 1) / 2;
    Canon k{};
    k.ssd = p->cost == WS_COST_SSD;
    if (is_census(p->cost) && p->view != WS_VIEW_LINEAR) return false; // (the census match kernel owns the whole map)
    if (p->view == WS_VIEW_LEFT) {
        k.wa = w1; k.ha = h1; k.wb = w2; k.hb = h2;
        k.ww = k.wh = p->block_size;
        k.wx0 = k.wy0 = -half;
        k.boff = 0;
        // no candidate beyond what the geometry allows (x - d >= half with x <= w1 - 1 - half): a range far
        // wider than the image costs neither d-group passes nor tie-tag bits; the tags keep their order
        k.d_lo = 1; k.d_hi = k.d_hi_clipped = std::min(p->max_disparity, w1 - 1 - 2 * half);
        k.b_lo = half; k.b_hi = w2 - half - 1;
        k.ox0 = half; k.ox1 = w1 - half;
        k.oy0 = half; k.oy1 = height - half;
        k.prefer_large = 1; k.mirror = 0; k.fallback_neg = 0;
    } else if (p->view == WS_VIEW_RIGHT) {
        if (half < 1) return false;
        k.wa = w2; k.ha = h2; k.wb = w1; k.hb = h1;
        k.ww = k.wh = 2 * half;
        k.wx0 = 1 - half; k.wy0 = -half;
        k.boff = w1 - w2;
        // (x + d + half < w1 with x >= half: the same clamp)
        k.d_lo = p->min_disparity; k.d_hi = std::min(p->max_disparity - 1, w1 - 1 - 2 * half);
        k.d_hi_clipped = std::min(p->max_disparity - 1, w1 - 1); // border ring: x >= 0 and right >= 0 only
        k.b_lo = half; k.b_hi = w1 - 1 - half;
        k.ox0 = half; k.ox1 = w2 - half;
        k.oy0 = half; k.oy1 = std::min(h2 - half, height);
        k.prefer_large = 0; k.mirror = 1; k.fallback_neg = 1;
    } else {
        return false;
    }
    *c = k;
    return k.ox1 > k.ox0 && k.oy1 > k.oy0 && k.d_hi >= k.d_lo;
}

// The wire format of a host call's map (see "WIRE FORMAT" in ws_staging.h): 16-bit integers when the search kernels can
// store them themselves and every value fits.  A search whose kernels only ever WRITE the map (smoothFactor 1, no
// sub-pixel refine, no varBlock: the marching kernel's flush, the border ring, LinearSearch, the brute force) can store
// it in the wire format itself.  Whatever the disparity range, a stored value is a difference of two columns of one
// image row or a +-x fallback (BlockSearch.cpp:82: x - cx with 0 <= cx < x; :174: cx - x with x <= cx < w1, or -x;
// LinearSearch.cpp:53: col - j), so |value| < max(w1, w2): images up to 32767 pixels wide fit.  Else float32.
int wire_for(const ws_params *p, const ws_image *L, const ws_image *R)
{
    if (p->view != WS_VIEW_LINEAR && is_census(p->cost)) return kWireF32; // (the match kernel stores float32 only)
    const bool writes_only = p->smooth_factor == 1.0 && !p->subpixel && !(p->var_block && p->view == WS_VIEW_RIGHT);
    const bool fits = L->width <= 32767 && R->width <= 32767;
    return writes_only && fits ? kWireI16 : kWireF32;
}

// The Searcher's scratch planes are shared by every search, under the Searcher's lease.
int search(Searcher &S, std::string *err, const ws_params *p, const ws_image *L, const ws_image *R, float *out,
           int out_stride, int16_t *out16, unsigned int *status, hipStream_t s)
{
    if (const int rc = S.lease.begin(err, s); rc != WS_OK) return rc;
    return S.lease.end(err, s, search_on(S, err, p, L, R, out, out_stride, out16, status, s));
}

} // namespace wsamd
