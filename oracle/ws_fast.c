/*
 * ws_fast.c -- fast exact CPU reference for BlockSearch (see ws_fast.h).
 *
 * TEST INFRASTRUCTURE ONLY.  The semantics are those of wso_block_left /
 * wso_block_right (ws_oracle.c, which names the reference lines); the route is
 * different:
 *
 *   col[x'][j]  exact integer sum, over the window's rows, of the pixel cost
 *               between B(y', x') and O(y', x' -/+ d), d = d0 + j
 *               (B: the image the map is indexed by -- L for the left view,
 *               R for the right view; O: the other one)
 *   win[j]      the window's sum: col slid along x' over the window's columns
 *
 * Every window of a row spans the same rows and its columns only move right as
 * x grows (also for the right view's clipped border windows), so both sums move
 * by entering and leaving rows / columns.  Sums wrap modulo 2^32 on the way but
 * every window sum is below 2^32 (checked up front), so the differences are
 * exact.  The pixel's candidates are a contiguous range of d; for smooth == 1
 * the winner is the first minimum of the integer sums in the reference's
 * candidate order (sqrt, and the division by a pixel's constant area, are
 * strictly increasing over the integers that occur), for smooth != 1 the
 * reference's double expressions are evaluated literally in a raster pass.
 */
#include "ws_fast.h"

#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

typedef struct {
    int right;                 /* 0: left view, 1: right view */
    const wso_image *B, *O;    /* B indexes the map, O is read at x' - d (left) / x' + d (right) */
    int cost, half;            /* half: (bs - 1) / 2, the right view's hb */
    int min_d, max_d;
    int w1, w2, h1, h2;
    int wb, wo;                /* widths of B and O */
    int d0, nd;                /* stored disparities: [d0, d0 + nd) */
    int ostride;               /* length of one O plane: wb + nd */
} geom;

typedef struct {
    uint32_t *col;             /* wb x nd (may be shared: callers own disjoint column ranges) */
    uint32_t *win;             /* nd */
    int32_t *planes;           /* two rows: B (3 x wb) and O (3 x ostride) each */
    int r0, r1;                /* rows col holds, [r0, r1); r0 < 0: nothing yet */
} work;

static inline const uint8_t *pix(const wso_image *im, int y, int x)
{
    return im->data + (size_t)y * (size_t)im->stride + (size_t)x * 3u;
}

static inline int black(const wso_image *im, int y, int x)
{
    const uint8_t *p = pix(im, y, x);
    return (p[0] | p[1] | p[2]) == 0;
}

/* rows of the window of output row y: [*a, *b) */
static inline void win_rows(const geom *g, int y, int *a, int *b)
{
    if (!g->right) {
        *a = y - g->half;
        *b = y + g->half + 1;
    } else {
        int up = y < g->half ? y : g->half;
        int down = g->h2 - y - 1 < g->half ? g->h2 - y - 1 : g->half;
        *a = y - up;
        *b = y + down;
    }
}

/* columns of the window of output column x: [*a, *b) */
static inline void win_cols(const geom *g, int x, int *a, int *b)
{
    if (!g->right) {
        *a = x - g->half;
        *b = x + g->half + 1;
    } else {
        int l = x < g->half ? x : g->half;
        int r = g->w2 - x - 1 < g->half ? g->w2 - x - 1 : g->half;
        *a = x - l;
        *b = x + r;
    }
}

/* Planar int32 copies of image row y: B at p[c * wb + x'], O at q[c * ostride + m] where
 * O's element for (x', j) sits at m = base(x') + j, base = wb - 1 - x' (left) or x' (right).
 * O columns outside the image read as 0 (no valid window ever covers them). */
static void load_row(const geom *g, int y, int32_t *p)
{
    int32_t *q = p + 3 * g->wb;
    for (int x = 0; x < g->wb; ++x) {
        const uint8_t *s = pix(g->B, y, x);
        p[x] = s[0];
        p[g->wb + x] = s[1];
        p[2 * g->wb + x] = s[2];
    }
    for (int m = 0; m < g->ostride; ++m) {
        int i = g->right ? m + g->d0 : (g->wb - 1 - g->d0) - m;
        int v0 = 0, v1 = 0, v2 = 0;
        if (i >= 0 && i < g->wo) {
            const uint8_t *s = pix(g->O, y, i);
            v0 = s[0];
            v1 = s[1];
            v2 = s[2];
        }
        q[m] = v0;
        q[g->ostride + m] = v1;
        q[2 * g->ostride + m] = v2;
    }
}

static inline int32_t ad(int32_t v) { return v < 0 ? -v : v; }

/* col[x'] += cost of row A (if a) - cost of row S (if s), for x' in [xa, xb) */
static void col_update(const geom *g, uint32_t *col, const int32_t *a, const int32_t *s, int xa, int xb)
{
    const int nd = g->nd, wb = g->wb, os = g->ostride;
    for (int x = xa; x < xb; ++x) {
        uint32_t *c = col + (size_t)x * nd;
        const int base = g->right ? x : wb - 1 - x;
        if (a && s) {
            const int32_t a0 = a[x], a1 = a[wb + x], a2 = a[2 * wb + x];
            const int32_t s0 = s[x], s1 = s[wb + x], s2 = s[2 * wb + x];
            const int32_t *p0 = a + 3 * wb + base, *p1 = p0 + os, *p2 = p1 + os;
            const int32_t *q0 = s + 3 * wb + base, *q1 = q0 + os, *q2 = q1 + os;
            if (g->cost == WSO_COST_SAD) {
                for (int j = 0; j < nd; ++j)
                    c[j] += (uint32_t)(ad(a0 - p0[j]) + ad(a1 - p1[j]) + ad(a2 - p2[j])
                                       - ad(s0 - q0[j]) - ad(s1 - q1[j]) - ad(s2 - q2[j]));
            } else {
                for (int j = 0; j < nd; ++j) {
                    int32_t e0 = a0 - p0[j], e1 = a1 - p1[j], e2 = a2 - p2[j];
                    int32_t f0 = s0 - q0[j], f1 = s1 - q1[j], f2 = s2 - q2[j];
                    c[j] += (uint32_t)(e0 * e0 + e1 * e1 + e2 * e2 - f0 * f0 - f1 * f1 - f2 * f2);
                }
            }
        } else {
            const int32_t *r = a ? a : s;
            const int32_t r0 = r[x], r1 = r[wb + x], r2 = r[2 * wb + x];
            const int32_t *p0 = r + 3 * wb + base, *p1 = p0 + os, *p2 = p1 + os;
            if (g->cost == WSO_COST_SAD) {
                if (a)
                    for (int j = 0; j < nd; ++j) c[j] += (uint32_t)(ad(r0 - p0[j]) + ad(r1 - p1[j]) + ad(r2 - p2[j]));
                else
                    for (int j = 0; j < nd; ++j) c[j] -= (uint32_t)(ad(r0 - p0[j]) + ad(r1 - p1[j]) + ad(r2 - p2[j]));
            } else {
                for (int j = 0; j < nd; ++j) {
                    int32_t e0 = r0 - p0[j], e1 = r1 - p1[j], e2 = r2 - p2[j];
                    uint32_t e = (uint32_t)(e0 * e0 + e1 * e1 + e2 * e2);
                    if (a)
                        c[j] += e;
                    else
                        c[j] -= e;
                }
            }
        }
    }
}

/* Move the column sums of [xa, xb) to the rows [n0, n1) (n0 >= r0 and n1 >= r1 once started). */
static void advance_rows(const geom *g, work *w, int n0, int n1, int xa, int xb)
{
    const size_t plane = (size_t)3 * g->wb + (size_t)3 * g->ostride;
    int32_t *pa = w->planes, *ps = w->planes + plane;
    if (w->r0 < 0 || n0 >= w->r1) {
        memset(w->col + (size_t)xa * g->nd, 0, sizeof(uint32_t) * (size_t)(xb - xa) * g->nd);
        w->r0 = w->r1 = n0;
    }
    while (w->r1 < n1 || w->r0 < n0) {
        int add = w->r1 < n1, sub = w->r0 < n0;
        if (add) load_row(g, w->r1, pa);
        if (sub) load_row(g, w->r0, ps);
        col_update(g, w->col, add ? pa : NULL, sub ? ps : NULL, xa, xb);
        w->r1 += add;
        w->r0 += sub;
    }
}

/* Slide win over the columns [*ca, *cb) to [a, b) (a >= *ca, b >= *cb). */
static void slide_cols(const geom *g, const uint32_t *col, uint32_t *win, int *ca, int *cb, int a, int b)
{
    const int nd = g->nd;
    if (a >= *cb) {
        memset(win, 0, sizeof(uint32_t) * (size_t)nd);
        *ca = *cb = a;
    }
    for (; *cb < b; ++*cb) {
        const uint32_t *c = col + (size_t)*cb * nd;
        for (int j = 0; j < nd; ++j) win[j] += c[j];
    }
    for (; *ca < a; ++*ca) {
        const uint32_t *c = col + (size_t)*ca * nd;
        for (int j = 0; j < nd; ++j) win[j] -= c[j];
    }
}

/* The candidates of pixel (x, y) as a range of d, [*lo, *hi]; 0 when there are none.  Left view:
 * cx = x - d in [x - max_d, x) with half <= cx < w2 - half (BlockSearch.cpp:53-57).  Right view:
 * cx = x + d from x + min_d until cx + right >= w1 (:147-149); the geometry error of :151-154 is
 * ruled out before the search.  A right-view window of zero area divides 0 by 0 (:158): no candidate. */
static int candidates(const geom *g, int x, int y, int *lo, int *hi)
{
    if (!g->right) {
        int a = x - g->w2 + g->half + 1, b = x - g->half;
        *lo = a > 1 ? a : 1;
        *hi = b < g->max_d ? b : g->max_d;
    } else {
        int l, r, t, u;
        win_cols(g, x, &l, &r);
        win_rows(g, y, &t, &u);
        if (r - l == 0 || u - t == 0) return 0;
        int b = g->w1 - 1 - (r - x) - x;
        *lo = g->min_d;
        *hi = b < g->max_d - 1 ? b : g->max_d - 1;
    }
    return *lo <= *hi;
}

/* First minimum in candidate order: largest d first (left view), smallest d first (right view). */
static int argmin_d(const geom *g, const uint32_t *win, int lo, int hi)
{
    const uint32_t *w = win - g->d0;
    uint32_t m = UINT32_MAX;
    for (int d = lo; d <= hi; ++d) m = w[d] < m ? w[d] : m;
    if (!g->right) {
        for (int d = hi; d > lo; --d)
            if (w[d] == m) return d;
        return lo;
    }
    for (int d = lo; d < hi; ++d)
        if (w[d] == m) return d;
    return hi;
}

/* the build's parabolic refinement of d, on the integer costs at d - 1, d, d + 1: the double sum, or for
 * WSO_SUBPIXEL_F32 the float32 value the device stores (the quotient rounded to float, one float addition) */
static double parabola(int d, uint32_t cm, uint32_t c0, uint32_t cp, int subpixel)
{
    double num = (double)cm - (double)cp;
    double den = (double)cm - 2.0 * (double)c0 + (double)cp;
    if (!(den > 0.0)) return (double)d;
    double q = num / (2.0 * den);
    if (subpixel != WSO_SUBPIXEL_F32) return (double)d + q;
    float f = (float)d + (float)q;
    return (double)f;
}

/* the reference's dist before smoothing: norm, and for the right view / (ww * wh) (:64-66, :156-158) */
static inline double dist_of(const geom *g, uint32_t c, int area)
{
    double v = g->cost == WSO_COST_SAD ? (double)c : sqrt((double)c);
    return g->right ? v / (double)area : v;
}

static inline int eligible(const geom *g, int y, int x)
{
    return !black(g->B, y, x);
}

/* Value with no candidate: best_cx = 0 (BlockSearch.cpp:50, :82, :174). */
static inline double fallback(const geom *g, int x) { return g->right ? (double)(0 - x) : (double)x; }

/* Output columns the search visits: [*xa, *xb). */
static void out_cols(const geom *g, int *xa, int *xb)
{
    *xa = g->right ? 0 : g->half;
    *xb = g->right ? g->w2 : g->w1 - g->half;
}

static int alloc_work(const geom *g, work *w, uint32_t *shared_col)
{
    const size_t plane = (size_t)3 * g->wb + (size_t)3 * g->ostride;
    w->col = shared_col ? shared_col : malloc(sizeof(uint32_t) * (size_t)g->wb * (size_t)(g->nd ? g->nd : 1));
    w->win = malloc(sizeof(uint32_t) * (size_t)(g->nd ? g->nd : 1));
    w->planes = malloc(sizeof(int32_t) * 2 * plane);
    w->r0 = w->r1 = -1;
    return w->col && w->win && w->planes;
}

static void free_work(work *w, int owns_col)
{
    if (owns_col) free(w->col);
    free(w->win);
    free(w->planes);
}

/* Can row y's windows be summed?  (The right view's rows past h1 never are: see the geometry check.) */
static inline int rows_readable(const geom *g, int y)
{
    int a, b;
    win_rows(g, y, &a, &b);
    return b <= g->h1 && b <= g->h2;
}

/* One output row, smooth == 1: every pixel's decision is independent. */
static void row_plain(const geom *g, work *w, int y, int subpixel, double *orow)
{
    int xa, xb;
    out_cols(g, &xa, &xb);
    const int readable = g->nd > 0 && rows_readable(g, y);
    if (readable) {
        int a, b;
        win_rows(g, y, &a, &b);
        advance_rows(g, w, a, b, 0, g->wb);
    }
    int ca = 0, cb = 0, started = 0;
    const uint32_t *wd = w->win - g->d0;
    for (int x = xa; x < xb; ++x) {
        if (!eligible(g, y, x)) continue;
        int lo, hi;
        if (!readable || !candidates(g, x, y, &lo, &hi)) {
            orow[x] = fallback(g, x);
            continue;
        }
        int a, b;
        win_cols(g, x, &a, &b);
        if (!started) {
            ca = cb = a;
            memset(w->win, 0, sizeof(uint32_t) * (size_t)g->nd);
            started = 1;
        }
        slide_cols(g, w->col, w->win, &ca, &cb, a, b);
        int d = argmin_d(g, w->win, lo, hi);
        orow[x] = subpixel && d > lo && d < hi ? parabola(d, wd[d - 1], wd[d], wd[d + 1], subpixel) : (double)d;
    }
}

/* wso_block_right's WSO_ERR_GEOMETRY: the first candidate of an eligible pixel passes the
 * cx + right < w1 test but its window leaves the left image (BlockSearch.cpp:147-154). */
static int right_geometry_error(const geom *g, int ya, int yb)
{
    if (g->max_d <= g->min_d) return 0;
    for (int y = ya; y < yb; ++y) {
        int ra, rb;
        win_rows(g, y, &ra, &rb);
        for (int x = 0; x < g->w2; ++x) {
            if (!eligible(g, y, x)) continue;
            int a, b;
            win_cols(g, x, &a, &b);
            long cx = (long)x + g->min_d;
            if (cx + (b - x) >= g->w1) continue;
            if (cx - (x - a) < 0 || rb > g->h1) return 1;
        }
    }
    return 0;
}

/* smooth != 1: rows in order; a row's window sums in parallel, then the reference's raster
 * decision with its double expressions (BlockSearch.cpp:64-79, :156-171). */
static int search_smooth(const geom *g, double smooth, int ya, int yb, double *out, int os, int threads)
{
    int xa, xb;
    out_cols(g, &xa, &xb);
    if (xb <= xa || yb <= ya) return WSO_OK;
    const int nd = g->nd ? g->nd : 1;
    if (threads > g->wb / 64) threads = g->wb / 64 > 1 ? g->wb / 64 : 1;   /* (a barrier per row and step) */
    uint32_t *col = malloc(sizeof(uint32_t) * (size_t)g->wb * nd);
    double *dist = malloc(sizeof(double) * (size_t)g->wb * nd);
    int err = !col || !dist;
#pragma omp parallel num_threads(threads) if (threads > 1) reduction(| : err)
    {
        int nt = 1, t = 0;
#ifdef _OPENMP
        nt = omp_get_num_threads();
        t = omp_get_thread_num();
#endif
        work w = {0};
        int ok = !err && alloc_work(g, &w, col);
        /* this thread's share of the column sums and of the pixels */
        const int c0 = (int)((long)g->wb * t / nt), c1 = (int)((long)g->wb * (t + 1) / nt);
        const int p0 = xa + (int)((long)(xb - xa) * t / nt), p1 = xa + (int)((long)(xb - xa) * (t + 1) / nt);
        for (int y = ya; y < yb; ++y) {
            const int readable = ok && g->nd > 0 && rows_readable(g, y);
            if (readable) {
                int a, b;
                win_rows(g, y, &a, &b);
                advance_rows(g, &w, a, b, c0, c1);
            }
#pragma omp barrier
            if (readable) {
                int ca = 0, cb = 0, started = 0;
                for (int x = p0; x < p1; ++x) {
                    int lo, hi, a, b;
                    if (!candidates(g, x, y, &lo, &hi)) continue;
                    win_cols(g, x, &a, &b);
                    if (!started) {
                        ca = cb = a;
                        memset(w.win, 0, sizeof(uint32_t) * (size_t)g->nd);
                        started = 1;
                    }
                    slide_cols(g, w.col, w.win, &ca, &cb, a, b);
                    double *dr = dist + (size_t)x * nd - g->d0;
                    const uint32_t *wd = w.win - g->d0;
                    int ra, rb;
                    win_rows(g, y, &ra, &rb);
                    const int area = (b - a) * (rb - ra);
                    for (int d = lo; d <= hi; ++d) dr[d] = dist_of(g, wd[d], area);
                }
            }
#pragma omp barrier
#pragma omp single
            {
                double *orow = out + (size_t)y * os;
                const double *up = y >= 1 ? out + (size_t)(y - 1) * os : NULL;
                for (int x = xa; x < xb; ++x) {
                    if (!eligible(g, y, x)) continue;
                    int lo, hi, found = 0, best_d = 0;
                    double best = DBL_MAX;
                    if (readable && candidates(g, x, y, &lo, &hi)) {
                        const double *dr = dist + (size_t)x * nd - g->d0;
                        const int step = g->right ? 1 : -1;
                        for (int d = g->right ? lo : hi; d >= lo && d <= hi; d += step) {
                            double v = dr[d];
                            const double dc = (double)(g->right ? -d : d);     /* (double)(x - cx) */
                            if (up && up[x] == dc) v *= smooth;
                            if (x >= 1 && orow[x - 1] == dc) v *= smooth;
                            if (v < best) {
                                best = v;
                                best_d = d;
                                found = 1;
                            }
                        }
                    }
                    orow[x] = found ? (double)best_d : fallback(g, x);
                }
            }
        }
        free_work(&w, 0);
        err |= !ok;
    }
    free(col);
    free(dist);
    return err ? WSO_ERR_ARG : WSO_OK;
}

/* smooth == 1: independent row bands, each restarting its sums. */
static int search_plain(const geom *g, int subpixel, int ya, int yb, double *out, int os, int threads)
{
    if (yb <= ya) return WSO_OK;
    const int rows = yb - ya;
    int nbands = threads > 1 ? 4 * threads : 1;
    if (nbands > rows / 32) nbands = rows / 32 > 1 ? rows / 32 : 1;   /* (every band re-sums its first window rows) */
    int err = 0;
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads) if (threads > 1) reduction(| : err)
    for (int k = 0; k < nbands; ++k) {
        work w;
        if (!alloc_work(g, &w, NULL)) {
            err = 1;
            free_work(&w, 1);
            continue;
        }
        const int b0 = ya + (int)((long)rows * k / nbands), b1 = ya + (int)((long)rows * (k + 1) / nbands);
        for (int y = b0; y < b1; ++y) row_plain(g, &w, y, subpixel, out + (size_t)y * os);
        free_work(&w, 1);
    }
    return err ? WSO_ERR_ARG : WSO_OK;
}

static int image_ok(const wso_image *im)
{
    return im && im->data && im->width > 0 && im->height > 0 && im->stride >= 3 * im->width;
}

static int threads_of(int threads)
{
#ifdef _OPENMP
    return threads < 1 ? omp_get_max_threads() : threads;
#else
    (void)threads;
    return 1;
#endif
}

/* Every window sum (and the plain path's column sums) must stay below 2^32. */
static int sums_fit(int ww, int wh, int cost)
{
    const double per = cost == WSO_COST_SAD ? 3.0 * 255.0 : 3.0 * 255.0 * 255.0;
    return per * (double)ww * (double)wh < 4294967296.0;
}

int wsf_block_left(const wso_image *L, const wso_image *R, int block_size,
                   int min_disparity, int max_disparity, double smooth,
                   int cost, int subpixel, int y0, int y1,
                   double *out, int out_stride, int threads)
{
    (void)min_disparity; /* never read by the reference's left view */
    if (!image_ok(L) || !image_ok(R) || !out || block_size < 1 ||
        out_stride < L->width || (cost != WSO_COST_SSD && cost != WSO_COST_SAD))
        return WSO_ERR_ARG;
    geom g;
    memset(&g, 0, sizeof g);
    g.right = 0;
    g.B = L;
    g.O = R;
    g.cost = cost;
    g.half = (block_size - 1) / 2;
    g.min_d = min_disparity;
    g.max_d = max_disparity;
    g.w1 = L->width, g.h1 = L->height, g.w2 = R->width, g.h2 = R->height;
    g.wb = g.w1, g.wo = g.w2;
    const int height = g.h1 < g.h2 ? g.h1 : g.h2;
    if (y0 < 0 || y1 > g.h1 || y0 > y1) return WSO_ERR_ARG;
    if (smooth != 1.0 && (y0 != 0 || subpixel)) return WSO_ERR_RANGE;
    if (!sums_fit(block_size, block_size, cost)) return WSF_ERR_UNSUPPORTED;

    for (int y = 0; y < g.h1; ++y) memset(out + (size_t)y * out_stride, 0, sizeof(double) * (size_t)g.w1);
    if ((block_size & 1) == 0 && height - 2 * g.half > 0 && g.w1 - 2 * g.half > 0)
        return WSO_ERR_GEOMETRY;

    /* d = x - cx runs over [1, max_d]; the largest any pixel can use is w1 - 1 - 2 half */
    int dmax = g.w1 - 1 - 2 * g.half;
    if (max_disparity < dmax) dmax = max_disparity;
    g.d0 = 1;
    g.nd = dmax >= 1 ? dmax : 0;
    g.ostride = g.wb + g.nd;
    const int ya = g.half > y0 ? g.half : y0;
    const int yb = height - g.half < y1 ? height - g.half : y1;
    threads = threads_of(threads);
    return smooth == 1.0 ? search_plain(&g, subpixel, ya, yb, out, out_stride, threads)
                         : search_smooth(&g, smooth, ya, yb, out, out_stride, threads);
}

/* ---- varBlock (BlockSearch.cpp:125-145): every right-view pixel its own window -------------------------------
 *
 * A route of its own, all sums 64-bit:
 *   texture  the window's per-channel value histogram, extended by the pixels a growth step adds (a window only
 *            grows), gives the exact integer channel sums (the mean) and the centred norm as sum over v of
 *            count[v] * clamp(rint((float)v - (float)mean))^2 -- the float32 subtraction depends on v alone;
 *            small windows are scanned directly instead
 *   costs    per disparity one summed-area table of the pixel cost over the right image's grid; a window's cost
 *            is four reads of it, whatever the window, O(H * W * D) in all
 *   decision smooth == 1: the first minimum of the integer costs in d order (sqrt and / area are strictly
 *            increasing over the sums that occur, checked below); smooth != 1: the raster pass with the
 *            reference's doubles -- the factor only reaches a d with -d equal to a neighbour's stored value, at
 *            most two per pixel, so the three best (cost, d) per pixel and the costs at those d decide it. */

typedef struct {
    int l, r, u, dn;           /* window extents about (x, y): columns [x - l, x + r), rows [y - u, y + dn) */
} vb_win;

/* the three best (cost, d) in lexicographic order; n of them valid */
typedef struct {
    uint64_t c[3];
    int d[3];
    int n;
} vb_top;

static inline void vb_clip(int w2, int h2, int x, int y, int bs, vb_win *w)
{
    const int hb = (bs - 1) / 2;
    w->l = x < hb ? x : hb;
    w->r = w2 - x - 1 < hb ? w2 - x - 1 : hb;
    w->u = y < hb ? y : hb;
    w->dn = h2 - y - 1 < hb ? h2 - y - 1 : hb;
}

typedef struct {
    int64_t hist[3][256];
    int64_t sum[3];
    int on;                    /* the histogram holds the window */
} vb_hist;

static void vb_hist_add(vb_hist *h, const wso_image *R, int xa, int xb, int ya, int yb)
{
    for (int y = ya; y < yb; ++y) {
        const uint8_t *p = pix(R, y, xa);
        for (int i = 0; i < xb - xa; ++i)
            for (int c = 0; c < 3; ++c) {
                h->hist[c][p[3 * i + c]]++;
                h->sum[c] += p[3 * i + c];
            }
    }
}

static inline int64_t vb_sq(float v, float fm)
{
    float fd = v - fm;
    long t = lrintf(fd);
    if (t < 0) t = 0;
    if (t > 255) t = 255;
    return (int64_t)(t * t);
}

/* cv::norm(window - cv::mean(window)) of w about (x, y), as wso_centred_norm defines it (ws_oracle.h). */
static double vb_texture(const wso_image *R, int x, int y, const vb_win *w, const vb_win *prev, vb_hist *h)
{
    const int ww = w->l + w->r, wh = w->u + w->dn;
    if (ww <= 0 || wh <= 0) return 0.0;
    const double n = (double)ww * (double)wh;
    if (ww * wh <= 96) {       /* small window: two direct passes */
        int64_t s[3] = {0, 0, 0};
        for (int yy = y - w->u; yy < y + w->dn; ++yy) {
            const uint8_t *p = pix(R, yy, x - w->l);
            for (int i = 0; i < ww; ++i)
                for (int c = 0; c < 3; ++c) s[c] += p[3 * i + c];
        }
        float fm[3];
        for (int c = 0; c < 3; ++c) fm[c] = (float)((double)s[c] / n);
        int64_t acc = 0;
        for (int yy = y - w->u; yy < y + w->dn; ++yy) {
            const uint8_t *p = pix(R, yy, x - w->l);
            for (int i = 0; i < ww; ++i)
                for (int c = 0; c < 3; ++c) acc += vb_sq((float)p[3 * i + c], fm[c]);
        }
        return sqrt((double)acc);
    }
    if (!h->on || !prev || prev->l + prev->r <= 0 || prev->u + prev->dn <= 0) {
        memset(h, 0, sizeof *h);
        vb_hist_add(h, R, x - w->l, x + w->r, y - w->u, y + w->dn);
        h->on = 1;
    } else {                   /* the ring the step added: full-width rows above / below, then the old rows' sides */
        vb_hist_add(h, R, x - w->l, x + w->r, y - w->u, y - prev->u);
        vb_hist_add(h, R, x - w->l, x + w->r, y + prev->dn, y + w->dn);
        vb_hist_add(h, R, x - w->l, x - prev->l, y - prev->u, y + prev->dn);
        vb_hist_add(h, R, x + prev->r, x + w->r, y - prev->u, y + prev->dn);
    }
    int64_t acc = 0;
    for (int c = 0; c < 3; ++c) {
        const float fm = (float)((double)h->sum[c] / n);
        for (int v = 0; v < 256; ++v)
            if (h->hist[c][v]) acc += h->hist[c][v] * vb_sq((float)v, fm);
    }
    return sqrt((double)acc);
}

/* The grown window of eligible pixel (x, y) and its block size (the last +4 counted, BlockSearch.cpp:129-145). */
static int vb_grow(const wso_image *R, int bs0, double thres, int x, int y, vb_win *w, vb_hist *h)
{
    const int w2 = R->width, h2 = R->height;
    int bs = bs0;
    vb_win prev;
    const vb_win *pp = NULL;
    vb_clip(w2, h2, x, y, bs, w);
    h->on = 0;
    while (vb_texture(R, x, y, w, pp, h) < thres) {
        vb_win g;
        bs += 4;
        vb_clip(w2, h2, x, y, bs, &g);
        if (g.l == w->l && g.r == w->r && g.u == w->u && g.dn == w->dn) break;
        prev = *w;
        pp = &prev;
        *w = g;
    }
    return bs;
}

static inline void vb_insert(vb_top *t, uint64_t c, int d, int k)
{
    /* d ascending: an equal cost ranks after every entry already held */
    int i = t->n < k ? t->n : k;
    if (i == k && !(c < t->c[k - 1])) return;
    if (i == k) --i;
    while (i > 0 && c < t->c[i - 1]) {
        t->c[i] = t->c[i - 1];
        t->d[i] = t->d[i - 1];
        --i;
    }
    t->c[i] = c;
    t->d[i] = d;
    if (t->n < k) t->n++;
}

/* the direct 64-bit window cost at d (the raster pass's factored candidates outside the captured ones) */
static uint64_t vb_cost_direct(const wso_image *L, const wso_image *R, int cost, int x, int y, const vb_win *w, int d)
{
    uint64_t acc = 0;
    for (int yy = y - w->u; yy < y + w->dn; ++yy) {
        const uint8_t *a = pix(L, yy, x + d - w->l), *b = pix(R, yy, x - w->l);
        for (int i = 0; i < 3 * (w->l + w->r); ++i) {
            int e = (int)a[i] - (int)b[i];
            acc += cost == WSO_COST_SAD ? (uint64_t)(e < 0 ? -e : e) : (uint64_t)(e * e);
        }
    }
    return acc;
}

static int var_block_right(const wso_image *L, const wso_image *R, int block_size, int min_d, int max_d,
                           double smooth, double thres, int cost, int y0, int y1, double *out, int os, int threads,
                           int *max_block_out)
{
    const int w1 = L->width, h1 = L->height, w2 = R->width, h2 = R->height;
    const int height = h1 < h2 ? h1 : h2;
    const int yb = height < y1 ? height : y1;
    const int rows = yb > y0 ? yb - y0 : 0;
    const size_t np = (size_t)rows * (size_t)w2;
    const int K = smooth == 1.0 ? 1 : 3;
    /* sqrt(c) / area strictly increasing over the sums that occur: c < 2^50 */
    const double per = cost == WSO_COST_SAD ? 3.0 * 255.0 : 3.0 * 255.0 * 255.0;
    if (per * (double)w2 * (double)h2 >= 1125899906842624.0) return WSF_ERR_UNSUPPORTED;

    vb_win *win = malloc(sizeof(vb_win) * (np ? np : 1));
    unsigned char *elig = malloc(np ? np : 1);
    vb_top *top = malloc(sizeof(vb_top) * (np ? np : 1));
    uint64_t *cap = malloc(sizeof(uint64_t) * 3 * (np ? np : 1));   /* costs at d = 0, x - 1, x */
    if (!win || !elig || !top || !cap) {
        free(win), free(elig), free(top), free(cap);
        return WSO_ERR_ARG;
    }
    int max_block = block_size, geometry_error = 0, err = 0;

    /* 1. windows */
#pragma omp parallel num_threads(threads) if (threads > 1) reduction(max : max_block) reduction(| : geometry_error, err)
    {
        vb_hist *h = malloc(sizeof(vb_hist));
        err |= !h;
#pragma omp for schedule(dynamic, 1)
        for (int y = y0; y < yb; ++y) {
            for (int x = 0; x < w2; ++x) {
                const size_t i = (size_t)(y - y0) * w2 + x;
                top[i].n = 0;
                cap[3 * i] = cap[3 * i + 1] = cap[3 * i + 2] = UINT64_MAX;
                elig[i] = !black(R, y, x);
                if (!elig[i]) continue;
                if (!h) continue;
                const int bs = vb_grow(R, block_size, thres, x, y, &win[i], h);
                if (bs > max_block) max_block = bs;
                /* the first candidate's window must lie in the left image (BlockSearch.cpp:147-154) */
                const long cx = (long)x + min_d;
                if (max_d > min_d && cx + win[i].r < w1 && (cx - win[i].l < 0 || y + win[i].dn > h1))
                    geometry_error = 1;
            }
        }
        free(h);
    }
    if (geometry_error || err) {
        free(win), free(elig), free(top), free(cap);
        return err ? WSO_ERR_ARG : WSO_ERR_GEOMETRY;
    }

    /* 2. costs: d over every candidate any pixel can have (cx - left >= 0 gives d >= 1 - w2, cx + right < w1 d < w1) */
    const int dlo = min_d > 1 - w2 ? min_d : 1 - w2;
    const int dhi = max_d - 1 < w1 - 1 ? max_d - 1 : w1 - 1;
    /* the table covers rows [0, height): every candidate's window has y + down <= h1 (checked above) and < h2 */
    const int sh = height, sw = w2 + 1;
    uint64_t *S = dhi >= dlo && rows ? malloc(sizeof(uint64_t) * (size_t)(sh + 1) * (size_t)sw) : NULL;
    err = dhi >= dlo && rows && !S;
    if (S) {
#pragma omp parallel num_threads(threads) if (threads > 1)
        for (int d = dlo; d <= dhi; ++d) {
#pragma omp for schedule(static)
            for (int y = 0; y <= sh; ++y) {
                uint64_t *s = S + (size_t)y * sw;
                s[0] = 0;
                if (y == 0) {
                    memset(s, 0, sizeof(uint64_t) * (size_t)sw);
                    continue;
                }
                const uint8_t *b = pix(R, y - 1, 0), *a = L->data + (size_t)(y - 1) * L->stride;
                uint64_t run = 0;
                for (int x = 0; x < w2; ++x) {
                    const int xl = x + d;
                    if (xl >= 0 && xl < w1) {
                        const uint8_t *p = a + 3 * (size_t)xl, *q = b + 3 * (size_t)x;
                        const int e0 = (int)p[0] - (int)q[0], e1 = (int)p[1] - (int)q[1], e2 = (int)p[2] - (int)q[2];
                        run += cost == WSO_COST_SAD ? (uint64_t)(abs(e0) + abs(e1) + abs(e2))
                                                    : (uint64_t)(e0 * e0 + e1 * e1 + e2 * e2);
                    }
                    s[x + 1] = run;
                }
            }
#pragma omp for schedule(static)
            for (int xa = 0; xa < sw; xa += 256) {
                const int xe = xa + 256 < sw ? xa + 256 : sw;
                for (int y = 2; y <= sh; ++y) {
                    uint64_t *s = S + (size_t)y * sw, *t = s - sw;
                    for (int x = xa; x < xe; ++x) s[x] += t[x];
                }
            }
#pragma omp for schedule(dynamic, 4)
            for (int y = y0; y < yb; ++y) {
                for (int x = 0; x < w2; ++x) {
                    const size_t i = (size_t)(y - y0) * w2 + x;
                    if (!elig[i]) continue;
                    const vb_win *w = &win[i];
                    if (w->l + w->r == 0 || w->u + w->dn == 0) continue;
                    if (d < min_d || x + d + w->r >= w1) continue;   /* not a candidate of this pixel */
                    const uint64_t *ra = S + (size_t)(y - w->u) * sw, *rb = S + (size_t)(y + w->dn) * sw;
                    const int ca = x - w->l, cb = x + w->r;
                    const uint64_t c = rb[cb] - rb[ca] - ra[cb] + ra[ca];
                    vb_insert(&top[i], c, d, K);
                    if (d == 0) cap[3 * i] = c;
                    if (d == x - 1) cap[3 * i + 1] = c;
                    if (d == x) cap[3 * i + 2] = c;
                }
            }
        }
    }
    free(S);

    /* 3. decisions */
    if (!err) {
        for (int y = y0; y < yb; ++y) {
            double *orow = out + (size_t)y * os;
            const double *up = y >= 1 ? out + (size_t)(y - 1) * os : NULL;
            for (int x = 0; x < w2; ++x) {
                const size_t i = (size_t)(y - y0) * w2 + x;
                if (!elig[i]) continue;
                const vb_top *t = &top[i];
                if (t->n == 0) {                              /* no candidate (or a zero-area window: 0/0) */
                    orow[x] = (double)(0 - x);
                    continue;
                }
                if (smooth == 1.0) {
                    orow[x] = (double)t->d[0];
                    continue;
                }
                const vb_win *w = &win[i];
                const int area = (w->l + w->r) * (w->u + w->dn);
                const int hi = max_d - 1 < w1 - 1 - w->r - x ? max_d - 1 : w1 - 1 - w->r - x;
                /* the d the factor reaches: -d == the stored value above / to the left (BlockSearch.cpp:160-165) */
                int fd[2], fk[2], nf = 0;
                const double nb[2] = {up ? up[x] : NAN, x >= 1 ? orow[x - 1] : NAN};
                for (int k = 0; k < 2; ++k) {
                    const double v = -nb[k];
                    if (!(v >= (double)min_d && v <= (double)hi)) continue;
                    const int d = (int)v;
                    if (nf == 1 && fd[0] == d) {
                        fk[0]++;
                        continue;
                    }
                    fd[nf] = d;
                    fk[nf++] = 1;
                }
                double best = DBL_MAX;
                int best_d = 0, found = 0;
                for (int j = 0; j < t->n; ++j) {             /* the best candidate the factor does not reach */
                    const int d = t->d[j];
                    if ((nf > 0 && fd[0] == d) || (nf > 1 && fd[1] == d)) continue;
                    best = (cost == WSO_COST_SAD ? (double)t->c[j] : sqrt((double)t->c[j])) / (double)area;
                    best_d = d;
                    found = 1;          /* (a window's dist is finite: below DBL_MAX) */
                    break;
                }
                for (int k = 0; k < nf; ++k) {
                    const int d = fd[k];
                    uint64_t c = d == 0 ? cap[3 * i] : d == x - 1 ? cap[3 * i + 1] : d == x ? cap[3 * i + 2] : UINT64_MAX;
                    if (c == UINT64_MAX) c = vb_cost_direct(L, R, cost, x, y, w, d);
                    double v = (cost == WSO_COST_SAD ? (double)c : sqrt((double)c)) / (double)area;
                    for (int m = 0; m < fk[k]; ++m) v *= smooth;
                    if (v < best || (v == best && found && d < best_d)) {
                        best = v;
                        best_d = d;
                        found = 1;
                    }
                }
                orow[x] = found ? (double)best_d : (double)(0 - x);
            }
        }
    }
    free(win), free(elig), free(top), free(cap);
    if (err) return WSO_ERR_ARG;
    if (max_block_out) *max_block_out = max_block;
    return WSO_OK;
}

int wsf_block_right_vb(const wso_image *L, const wso_image *R, int block_size,
                       int min_disparity, int max_disparity, double smooth,
                       int var_block, double thres, int cost, int subpixel, int y0, int y1,
                       double *out, int out_stride, int *max_block_out, int threads)
{
    if (!image_ok(L) || !image_ok(R) || !out || block_size < 1 ||
        out_stride < R->width || (cost != WSO_COST_SSD && cost != WSO_COST_SAD))
        return WSO_ERR_ARG;
    geom g;
    memset(&g, 0, sizeof g);
    g.right = 1;
    g.B = R;
    g.O = L;
    g.cost = cost;
    g.half = (block_size - 1) / 2;
    g.min_d = min_disparity;
    g.max_d = max_disparity;
    g.w1 = L->width, g.h1 = L->height, g.w2 = R->width, g.h2 = R->height;
    g.wb = g.w2, g.wo = g.w1;
    const int height = g.h1 < g.h2 ? g.h1 : g.h2;
    if (y0 < 0 || y1 > g.h2 || y0 > y1) return WSO_ERR_ARG;
    if (smooth != 1.0 && (y0 != 0 || subpixel)) return WSO_ERR_RANGE;
    if (var_block && subpixel) return WSF_ERR_UNSUPPORTED;
    if (!var_block && !sums_fit(2 * g.half, 2 * g.half, cost)) return WSF_ERR_UNSUPPORTED;

    for (int y = 0; y < g.h2; ++y) memset(out + (size_t)y * out_stride, 0, sizeof(double) * (size_t)g.w2);
    threads = threads_of(threads);
    if (var_block)
        return var_block_right(L, R, block_size, min_disparity, max_disparity, smooth, thres, cost, y0, y1, out,
                               out_stride, threads, max_block_out);
    const int yb = height < y1 ? height : y1;
    if (right_geometry_error(&g, y0, yb)) return WSO_ERR_GEOMETRY;

    /* d = cx - x runs over [min_d, max_d); cx + right < w1 caps it at w1 - 1, and a pixel whose
     * first candidate passes that test reads from cx - left >= 0, so d >= -(w2 - 1) */
    int dlo = min_disparity > 1 - g.w2 ? min_disparity : 1 - g.w2;
    int dhi = max_disparity - 1 < g.w1 - 1 ? max_disparity - 1 : g.w1 - 1;
    g.d0 = dlo;
    g.nd = dhi >= dlo ? dhi - dlo + 1 : 0;
    g.ostride = g.wb + g.nd;
    int rc = smooth == 1.0 ? search_plain(&g, subpixel, y0, yb, out, out_stride, threads)
                           : search_smooth(&g, smooth, y0, yb, out, out_stride, threads);
    if (rc == WSO_OK && max_block_out) *max_block_out = block_size;
    return rc;
}

int wsf_block_right(const wso_image *L, const wso_image *R, int block_size,
                    int min_disparity, int max_disparity, double smooth,
                    int var_block, int cost, int subpixel, int y0, int y1,
                    double *out, int out_stride, int threads)
{
    if (!image_ok(L) || !image_ok(R) || !out || block_size < 1 ||
        out_stride < R->width || (cost != WSO_COST_SSD && cost != WSO_COST_SAD))
        return WSO_ERR_ARG;
    if (var_block) return WSF_ERR_UNSUPPORTED;   /* (no thres here: wsf_block_right_vb) */
    return wsf_block_right_vb(L, R, block_size, min_disparity, max_disparity, smooth, 0, 0.0, cost, subpixel, y0, y1,
                              out, out_stride, NULL, threads);
}
