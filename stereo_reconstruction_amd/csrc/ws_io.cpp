// ws_io.cpp -- the Middlebury plumbing of include/ws_stereo.h (host only): PFM / PPM, calib.txt, OFF mesh, evaldisp.
#include "../../include/ws_stereo.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <string>
#include <vector>

extern "C" {

void ws_free(void *p) { free(p); }

int ws_pfm_read(const char *path, float **data, int *width, int *height)
{
    if (!path || !data || !width || !height) return WS_ERR_ARG;
    FILE *f = fopen(path, "rb");
    if (!f) return WS_ERR_IO;
    char tag[8] = {0};
    int w = 0, h = 0;
    double scale = 0;
    // "Pf" = one channel; header fields are whitespace separated, one whitespace byte before data
    if (fscanf(f, "%7s %d %d %lf", tag, &w, &h, &scale) != 4 || strcmp(tag, "Pf") != 0 || w <= 0 || h <= 0 ||
        scale == 0) {
        fclose(f);
        return WS_ERR_IO;
    }
    fgetc(f);
    float *buf = static_cast<float *>(malloc((size_t)w * h * sizeof(float)));
    if (!buf) { fclose(f); return WS_ERR_NOMEM; }
    const uint16_t probe = 1;
    const bool host_little = *reinterpret_cast<const uint8_t *>(&probe) == 1;
    const bool file_little = scale < 0;
    for (int y = h - 1; y >= 0; --y) { // the file stores the bottom row first
        float *row = buf + (size_t)y * w;
        if (fread(row, sizeof(float), (size_t)w, f) != (size_t)w) { free(buf); fclose(f); return WS_ERR_IO; }
        if (host_little != file_little)
            for (int x = 0; x < w; ++x) {
                uint32_t v;
                memcpy(&v, row + x, 4);
                v = (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
                memcpy(row + x, &v, 4);
            }
    }
    fclose(f);
    *data = buf; *width = w; *height = h;
    return WS_OK;
}

int ws_pfm_write(const char *path, const float *data, int width, int height, int stride)
{
    if (!path || !data || width <= 0 || height <= 0 || stride < width) return WS_ERR_ARG;
    FILE *f = fopen(path, "wb");
    if (!f) return WS_ERR_IO;
    const uint16_t probe = 1;
    const bool host_little = *reinterpret_cast<const uint8_t *>(&probe) == 1;
    fprintf(f, "Pf\n%d %d\n%s\n", width, height, host_little ? "-1.0" : "1.0");
    for (int y = height - 1; y >= 0; --y)
        if (fwrite(data + (size_t)y * stride, sizeof(float), (size_t)width, f) != (size_t)width) { fclose(f); return WS_ERR_IO; }
    return fclose(f) == 0 ? WS_OK : WS_ERR_IO;
}

// Binary PPM ("P6", maxval 255) <-> BGR rows, standing in for cv::imread(IMREAD_COLOR) / imwrite
// of the reference's PNGs (data_loader.cpp:71-72): no PNG decoder is linked here.
int ws_ppm_read(const char *path, uint8_t **bgr, int *width, int *height)
{
    if (!path || !bgr || !width || !height) return WS_ERR_ARG;
    FILE *f = fopen(path, "rb");
    if (!f) return WS_ERR_IO;
    char tag[3] = {0};
    int vals[3], n = 0;
    if (fread(tag, 1, 2, f) != 2 || tag[0] != 'P' || tag[1] != '6') { fclose(f); return WS_ERR_IO; }
    while (n < 3) { // width, height, maxval with '#' comments allowed between them
        int c = fgetc(f);
        if (c == EOF) { fclose(f); return WS_ERR_IO; }
        if (c == '#') { while (c != '\n' && c != EOF) c = fgetc(f); continue; }
        if (c == ' ' || c == '\t' || c == '\n' || c == '\r') continue;
        ungetc(c, f);
        if (fscanf(f, "%d", &vals[n]) != 1) { fclose(f); return WS_ERR_IO; }
        ++n;
    }
    fgetc(f); // the single whitespace byte before the pixels
    const int w = vals[0], h = vals[1];
    if (w <= 0 || h <= 0 || vals[2] != 255) { fclose(f); return WS_ERR_IO; }
    uint8_t *buf = static_cast<uint8_t *>(malloc((size_t)w * h * 3));
    if (!buf) { fclose(f); return WS_ERR_NOMEM; }
    if (fread(buf, 3, (size_t)w * h, f) != (size_t)w * h) { free(buf); fclose(f); return WS_ERR_IO; }
    fclose(f);
    for (size_t i = 0; i < (size_t)w * h; ++i) std::swap(buf[3 * i], buf[3 * i + 2]); // RGB -> BGR
    *bgr = buf; *width = w; *height = h;
    return WS_OK;
}

int ws_ppm_write(const char *path, const uint8_t *bgr, int width, int height, int stride)
{
    if (!path || !bgr || width <= 0 || height <= 0 || stride < 3 * width) return WS_ERR_ARG;
    FILE *f = fopen(path, "wb");
    if (!f) return WS_ERR_IO;
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    std::vector<uint8_t> row((size_t)width * 3);
    for (int y = 0; y < height; ++y) {
        const uint8_t *p = bgr + (size_t)y * stride;
        for (int x = 0; x < width; ++x) { row[3 * x] = p[3 * x + 2]; row[3 * x + 1] = p[3 * x + 1]; row[3 * x + 2] = p[3 * x]; }
        if (fwrite(row.data(), 1, row.size(), f) != row.size()) { fclose(f); return WS_ERR_IO; }
    }
    return fclose(f) == 0 ? WS_OK : WS_ERR_IO;
}

static bool parse_cam(const char *line, float m[9])
{
    // "cam0=[fx 0 cx; 0 fy cy; 0 0 1]": drop 6 leading characters and the closing bracket,
    // semicolons become blanks (data_loader.cpp:148-154)
    std::string s(line);
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
    if (s.size() < 8) return false;
    s = s.substr(6, s.size() - 7);
    std::replace(s.begin(), s.end(), ';', ' ');
    return sscanf(s.c_str(), "%f %f %f %f %f %f %f %f %f", m, m + 1, m + 2, m + 3, m + 4, m + 5, m + 6, m + 7, m + 8) == 9;
}

// WriteMesh (reconstruction.cpp:72-149) with CheckTriangularValidity (:46-69): COFF text, every
// vertex written (invalid ones as "0 0 0"), two triangles per grid cell when all three corners are
// valid and every edge is at most edge_threshold long.  Host only: file I/O bound.
static bool mesh_triangle_ok(const float *pos, unsigned a, unsigned b, unsigned c, float thr)
{
    const float minf = -INFINITY;
    if (pos[4 * a] == minf || pos[4 * b] == minf || pos[4 * c] == minf) return false;
    auto len = [&](unsigned p, unsigned q) {
        return sqrtf(powf(pos[4 * p] - pos[4 * q], 2) + powf(pos[4 * p + 1] - pos[4 * q + 1], 2) +
                     powf(pos[4 * p + 2] - pos[4 * q + 2], 2));
    };
    return !(len(a, b) > thr || len(a, c) > thr || len(b, c) > thr);
}

int ws_write_mesh_off(const char *path, const float *positions, const uint8_t *colors, int width, int height,
                      float edge_threshold)
{
    if (!path || !positions || !colors || width <= 0 || height <= 0) return WS_ERR_ARG;
    std::vector<unsigned> tri;
    const unsigned w = (unsigned)width, h = (unsigned)height;
    for (unsigned y = 0; y + 1 < h; ++y)
        for (unsigned x = 0; x + 1 < w; ++x) {
            const unsigned i00 = y * w + x, i10 = (y + 1) * w + x, i01 = y * w + x + 1, i11 = (y + 1) * w + x + 1;
            if (mesh_triangle_ok(positions, i00, i10, i01, edge_threshold)) { tri.push_back(i00); tri.push_back(i10); tri.push_back(i01); }
            if (mesh_triangle_ok(positions, i10, i11, i01, edge_threshold)) { tri.push_back(i10); tri.push_back(i11); tri.push_back(i01); }
        }
    std::ofstream out(path);
    if (!out.is_open()) return WS_ERR_IO;
    out << "COFF" << std::endl;
    out << (size_t)w * h << " " << tri.size() / 3 << " 0" << std::endl;
    const float minf = -INFINITY;
    for (size_t n = 0; n < (size_t)w * h; ++n) {
        if (positions[4 * n] == minf) out << "0 0 0 ";
        else out << positions[4 * n] << " " << positions[4 * n + 1] << " " << positions[4 * n + 2] << " ";
        out << (unsigned)colors[4 * n] << " " << (unsigned)colors[4 * n + 1] << " " << (unsigned)colors[4 * n + 2] << " "
            << (unsigned)colors[4 * n + 3] << std::endl;
    }
    for (size_t n = 0; n < tri.size() / 3; ++n)
        out << "3 " << tri[3 * n] << " " << tri[3 * n + 1] << " " << tri[3 * n + 2] << std::endl;
    out.close();
    return out.fail() ? WS_ERR_IO : WS_OK;
}

int ws_calib_read(const char *path, ws_calib *out)
{
    if (!path || !out) return WS_ERR_ARG;
    FILE *f = fopen(path, "r");
    if (!f) return WS_ERR_IO;
    memset(out, 0, sizeof *out);
    out->doffs = out->baseline = -1.0f;
    out->width = out->height = out->ndisp = -1;
    char line[512];
    int n = 0;
    bool ok = true;
    while (fgets(line, sizeof line, f)) {
        if (n == 0) ok = ok && parse_cam(line, out->cam0);
        else if (n == 1) ok = ok && parse_cam(line, out->cam1);
        else {
            float v;
            if (sscanf(line, "doffs=%f", &v) == 1) out->doffs = v;
            else if (sscanf(line, "baseline=%f", &v) == 1) out->baseline = v;
            else if (sscanf(line, "width=%f", &v) == 1) out->width = (int)v;
            else if (sscanf(line, "height=%f", &v) == 1) out->height = (int)v;
            else if (sscanf(line, "ndisp=%f", &v) == 1) out->ndisp = (int)v;
        }
        ++n;
    }
    fclose(f);
    return (ok && n >= 2) ? WS_OK : WS_ERR_IO;
}

int ws_evaldisp(const float *disp, const float *gt, const uint8_t *mask, int width, int height,
                float badthresh, float maxdisp, int rounddisp, double res[6])
{
    if (!disp || !gt || !mask || !res || width <= 0 || height <= 0) return WS_ERR_ARG;
    int n = 0, bad = 0, invalid = 0;
    float serr = 0;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t o = (size_t)y * width + x;
            const float g = gt[o];
            if (g == INFINITY) continue;                    // unknown (utils.cpp:137)
            float d = disp[o];
            const bool valid = d != 0;                      // utils.cpp:140
            if (valid) d = fmaxf(0.0f, fminf(maxdisp, d));
            if (valid && rounddisp) d = roundf(d);
            const float err = fabsf(d - g);
            if (mask[o] != 255) continue;                   // utils.cpp:146
            ++n;
            if (valid) { serr += err; if (err > badthresh) ++bad; }
            else ++invalid;
        }
    res[0] = n;
    res[1] = (float)(100.0 * bad / n);
    res[2] = (float)(100.0 * invalid / n);
    res[3] = (float)(100.0 * (bad + invalid) / n);
    res[4] = serr / (float)(n - invalid);
    res[5] = 100.0 * n / ((double)width * height);
    return WS_OK;
}

} // extern "C"
