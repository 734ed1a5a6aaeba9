// window_search.hpp -- C++ facade over the C-ABI (include/ws_stereo.h) with the reference's
// class and method names, so that the call sites of the reference keep reading the same:
//
//   reference (src/WindowSearch/BlockSearch.h:9-46, LinearSearch.h:9-20,
//              src/Rectification/rectification.hpp:50-51,64-66, rectification.cpp:66-88)
//       auto bs  = BlockSearch(leftRectified, rightRectified, blockSize, minD, maxD);
//       cv::Mat d = bs.computeDisparityMapLeft(smoothFactor);            // CV_64F
//   here
//       auto bs  = wsamd::BlockSearch(wsamd::view(left), wsamd::view(right), blockSize, minD, maxD);
//       wsamd::MatF64 d = bs.computeDisparityMapLeft(smoothFactor);      // doubles, row-major
//
// An unrectified pair goes through ImageRectifier (rectification.cpp:66-88, :432-505): the image warps, the search
// and the warp back in one device call.
//
// Header only; link against libws_stereo.so.  Errors the reference raises as cv::Exception
// (even blockSize, ROI outside the image) and everything the device cannot run surface as
// wsamd::Error.  Define WSAMD_WITH_OPENCV before including to get cv::Mat adapters.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ws_stereo.h"

#ifdef WSAMD_WITH_OPENCV
#include <opencv2/core.hpp>
#endif

namespace wsamd {

class Error : public std::runtime_error {
public:
    Error(int code, const std::string &what) : std::runtime_error(what), code_(code) {}
    int code() const { return code_; }

private:
    int code_;
};

// A CV_8UC3 image header on caller-owned pixels (what a cv::Mat header is to BlockSearch).
struct Image8UC3 {
    const uint8_t *data = nullptr;
    int rows = 0, cols = 0;
    size_t step = 0; // bytes per row
};

inline Image8UC3 view(const uint8_t *bgr, int rows, int cols, size_t step = 0)
{
    Image8UC3 v;
    v.data = bgr;
    v.rows = rows;
    v.cols = cols;
    v.step = step ? step : static_cast<size_t>(cols) * 3;
    return v;
}

// A CV_64F map owned by value, as the reference's methods return it (BlockSearch.cpp:33,85).
class MatF64 {
public:
    MatF64() = default;
    MatF64(int rows, int cols) : rows(rows), cols(cols), buf_(static_cast<size_t>(rows) * cols, 0.0) {}
    int rows = 0, cols = 0;
    double &at(int y, int x) { return buf_[static_cast<size_t>(y) * cols + x]; }
    double at(int y, int x) const { return buf_[static_cast<size_t>(y) * cols + x]; }
    double *ptr() { return buf_.data(); }
    const double *ptr() const { return buf_.data(); }
    bool empty() const { return buf_.empty(); }

private:
    std::vector<double> buf_;
};

// One ws_context per device, shared by the objects created on that device.
class Device {
public:
    explicit Device(int index = 0)
    {
        ws_context *c = nullptr;
        const int rc = ws_create(index, &c);
        if (rc != WS_OK) throw Error(rc, ws_last_error(nullptr));
        ctx_.reset(c, ws_destroy);
    }
    ws_context *get() const { return ctx_.get(); }
    static Device &shared()
    {
        static Device d(0);
        return d;
    }

private:
    std::shared_ptr<ws_context> ctx_;
};

namespace detail {
inline ws_image to_c(const Image8UC3 &m)
{
    ws_image im;
    im.data = m.data;
    im.width = m.cols;
    im.height = m.rows;
    im.stride = static_cast<int>(m.step);
    return im;
}
inline MatF64 run(Device &dev, const ws_params &p, const Image8UC3 &l, const Image8UC3 &r)
{
    const bool left = p.view == WS_VIEW_LEFT;
    MatF64 out(left ? l.rows : r.rows, left ? l.cols : r.cols);
    const ws_image li = to_c(l), ri = to_c(r);
    const int rc = ws_search_host(dev.get(), &p, &li, &ri, out.ptr(), out.cols, WS_OUT_F64);
    if (rc != WS_OK) throw Error(rc, ws_last_error(dev.get()));
    return out;
}
} // namespace detail

// BlockSearch (BlockSearch.h:9-46).  `cost` and `subpixel` are the build's extensions.
class BlockSearch {
public:
    BlockSearch(const Image8UC3 &leftImage, const Image8UC3 &rightImage, int blockSize,
                int minDisparity, int maxDisparity, Device &device = Device::shared())
        : leftImage_(leftImage), rightImage_(rightImage), blockSize_(blockSize),
          maxDisparity_(maxDisparity), minDisparity_(minDisparity), device_(device)
    {
    }

    int cost = WS_COST_SSD; // the reference's NORM_L2; WS_COST_SAD, or WS_COST_CENSUS_5X5 / WS_COST_CENSUS_9X7 (the Hamming
                            // distance of census-transform descriptors, smoothFactor 1 only; rules in ws_stereo.h)
    bool subpixel = false;

    MatF64 computeDisparityMapLeft(double smoothFactor) // BlockSearch.cpp:24-86
    {
        ws_params p = params(WS_VIEW_LEFT, smoothFactor);
        return detail::run(device_, p, leftImage_, rightImage_);
    }

    MatF64 computeDisparityMapRight(double smoothFactor, bool varBlock = false,
                                    double thres = 19.0) // BlockSearch.cpp:88-179
    {
        ws_params p = params(WS_VIEW_RIGHT, smoothFactor);
        p.var_block = varBlock;
        p.thres = thres;
        return detail::run(device_, p, leftImage_, rightImage_);
    }

    // Extension: computeDisparityMapLeft(smoothFactor) and computeDisparityMapRight(smoothFactor, varBlock, thres) in one
    // call, then the left-right check (OpenCV's disp12MaxDiff = maxDiff; rules in ws_stereo.h).  {left map, right map}:
    // a failed pixel is 0 (no disparity), or with fill the farther of the nearest passed pixels of its row.
    std::pair<MatF64, MatF64> computeDisparityMapsChecked(double smoothFactor, float maxDiff = 1.0f, bool fill = false,
                                                          bool varBlock = false, double thres = 19.0)
    {
        ws_params p = params(WS_VIEW_LEFT, smoothFactor);
        p.var_block = varBlock;
        p.thres = thres;
        ws_lr_params lr;
        lr.max_diff = maxDiff;
        lr.fill = fill ? WS_LR_FILL_BACKGROUND : WS_LR_FILL_NONE;
        std::pair<MatF64, MatF64> out(MatF64(leftImage_.rows, leftImage_.cols), MatF64(rightImage_.rows, rightImage_.cols));
        const ws_image li = detail::to_c(leftImage_), ri = detail::to_c(rightImage_);
        const int rc = ws_search_lr_host(device_.get(), &p, &li, &ri, &lr, out.first.ptr(), out.first.cols, out.second.ptr(),
                                         out.second.cols, WS_OUT_F64);
        if (rc != WS_OK) throw Error(rc, ws_last_error(device_.get()));
        return out;
    }

    // Extension: semi-global matching over the window costs of computeDisparityMapLeft(1) / computeDisparityMapRight(1)
    // (rules in ws_stereo.h): P1 and P2 in cost units, 4 or 8 paths.  With P1 = P2 = 0 the maps are those two calls'.
    MatF64 computeDisparityMapLeftSGM(int P1, int P2, int paths = 8) { return sgm(WS_VIEW_LEFT, P1, P2, paths); }
    MatF64 computeDisparityMapRightSGM(int P1, int P2, int paths = 8) { return sgm(WS_VIEW_RIGHT, P1, P2, paths); }

    // Extension: OpenCV's uniquenessRatio (rules in ws_stereo.h).  The maps of computeDisparityMapLeft(1) /
    // computeDisparityMapRight(1), or with paths = 4 or 8 those of the SGM calls above, with every pixel whose best cost
    // does not beat its best rival (two or more disparities away) by uniquenessRatio percent set to 0, no disparity.
    // confidence, if not null, receives the margin itself: float32, the map's size, 1 = unrivalled, 0 = a tie.
    MatF64 computeDisparityMapLeftUnique(int uniquenessRatio, std::vector<float> *confidence = nullptr, int paths = 0, int P1 = 0,
                                         int P2 = 0)
    {
        return unique(WS_VIEW_LEFT, uniquenessRatio, confidence, paths, P1, P2);
    }
    MatF64 computeDisparityMapRightUnique(int uniquenessRatio, std::vector<float> *confidence = nullptr, int paths = 0, int P1 = 0,
                                          int P2 = 0)
    {
        return unique(WS_VIEW_RIGHT, uniquenessRatio, confidence, paths, P1, P2);
    }

    // Extension: semi-global matching of one view (baseLeft: the left one), the other view's map derived from the same
    // sums, and the left-right check of the two in one call (rules in ws_stereo.h, "both views from one volume").
    // {left map, right map}, as computeDisparityMapsChecked returns them.  uniquenessRatio < 0: no ratio test, else
    // the test of computeDisparityMap*Unique on the base view's winner.
    std::pair<MatF64, MatF64> computeDisparityMapsCheckedSGM(int P1, int P2, int paths = 8, float maxDiff = 1.0f, bool fill = false,
                                                             int uniquenessRatio = -1, bool baseLeft = true)
    {
        const ws_params p = params(baseLeft ? WS_VIEW_LEFT : WS_VIEW_RIGHT, 1.0);
        ws_sgm_params sp;
        sp.paths = paths;
        sp.p1 = P1;
        sp.p2 = P2;
        ws_unique_params uq;
        uq.ratio = uniquenessRatio;
        ws_lr_params lr;
        lr.max_diff = maxDiff;
        lr.fill = fill ? WS_LR_FILL_BACKGROUND : WS_LR_FILL_NONE;
        std::pair<MatF64, MatF64> out(MatF64(leftImage_.rows, leftImage_.cols), MatF64(rightImage_.rows, rightImage_.cols));
        const ws_image li = detail::to_c(leftImage_), ri = detail::to_c(rightImage_);
        const int rc = ws_search_pair_host(device_.get(), &p, &sp, uniquenessRatio < 0 ? nullptr : &uq, &lr, &li, &ri, out.first.ptr(),
                                           out.first.cols, out.second.ptr(), out.second.cols, WS_OUT_F64);
        if (rc != WS_OK) throw Error(rc, ws_last_error(device_.get()));
        return out;
    }

private:
    MatF64 unique(int view, int ratio, std::vector<float> *confidence, int paths, int P1, int P2)
    {
        const ws_params p = params(view, 1.0);
        ws_sgm_params sp;
        sp.paths = paths;
        sp.p1 = P1;
        sp.p2 = P2;
        ws_unique_params uq;
        uq.ratio = ratio;
        const bool left = view == WS_VIEW_LEFT;
        MatF64 out(left ? leftImage_.rows : rightImage_.rows, left ? leftImage_.cols : rightImage_.cols);
        if (confidence) confidence->assign(static_cast<size_t>(out.rows) * out.cols, 0.0f);
        const ws_image li = detail::to_c(leftImage_), ri = detail::to_c(rightImage_);
        const int rc = ws_search_unique_host(device_.get(), &p, paths ? &sp : nullptr, &uq, &li, &ri, out.ptr(), out.cols, WS_OUT_F64,
                                             confidence ? confidence->data() : nullptr, out.cols);
        if (rc != WS_OK) throw Error(rc, ws_last_error(device_.get()));
        return out;
    }

    MatF64 sgm(int view, int P1, int P2, int paths)
    {
        const ws_params p = params(view, 1.0);
        ws_sgm_params sp;
        sp.paths = paths;
        sp.p1 = P1;
        sp.p2 = P2;
        const bool left = view == WS_VIEW_LEFT;
        MatF64 out(left ? leftImage_.rows : rightImage_.rows, left ? leftImage_.cols : rightImage_.cols);
        const ws_image li = detail::to_c(leftImage_), ri = detail::to_c(rightImage_);
        const int rc = ws_search_sgm_host(device_.get(), &p, &sp, &li, &ri, out.ptr(), out.cols, WS_OUT_F64);
        if (rc != WS_OK) throw Error(rc, ws_last_error(device_.get()));
        return out;
    }

    ws_params params(int view, double smoothFactor) const
    {
        ws_params p;
        ws_params_default(&p);
        p.view = view;
        p.cost = cost;
        p.block_size = blockSize_;
        p.min_disparity = minDisparity_;
        p.max_disparity = maxDisparity_;
        p.smooth_factor = smoothFactor;
        p.subpixel = subpixel;
        return p;
    }
    Image8UC3 leftImage_, rightImage_;
    int blockSize_, maxDisparity_, minDisparity_;
    Device &device_;
};

// LinearSearch (LinearSearch.h:9-20).
class LinearSearch {
public:
    LinearSearch(const Image8UC3 &leftImage, const Image8UC3 &rightImage,
                 Device &device = Device::shared())
        : leftImage(leftImage), rightImage(rightImage), device_(device)
    {
    }
    MatF64 computeDisparityMap(double smoothFactor) // LinearSearch.cpp:10-59
    {
        ws_params p;
        ws_params_default(&p);
        p.view = WS_VIEW_LINEAR;
        p.smooth_factor = smoothFactor;
        return detail::run(device_, p, leftImage, rightImage);
    }

private:
    Image8UC3 leftImage, rightImage;
    Device &device_;
};

// The boundary methods of ImageRectifier (rectification.cpp:66-88, getters :515-521): block search
// on the rectified pair, then cv::warpPerspective(map, H_.inv(), original size, INTER_NEAREST) back
// to the original frame (the reference uses H_ for both views).  For pairs that are already
// rectified (Middlebury) leave H at the identity: the warp is then a copy and is skipped.
class RectifiedPair {
public:
    RectifiedPair(const Image8UC3 &leftRectified, const Image8UC3 &rightRectified,
                  Device &device = Device::shared())
        : left_(leftRectified), right_(rightRectified), device_(device)
    {
    }
    // H = the rectifying homography H_ (row-major 3x3); rows/cols = size of the original images
    void setHomography(const double H[9], int leftRows, int leftCols, int rightRows, int rightCols)
    {
        for (int i = 0; i < 9; ++i) H_[i] = H[i];
        rows_[0] = leftRows; cols_[0] = leftCols; rows_[1] = rightRows; cols_[1] = rightCols;
        warp_ = true;
    }
    void computeDisparityMapLeft(int blockSize, int minDisparity, int maxDisparity, double smoothFactor)
    {
        MatF64 rect = BlockSearch(left_, right_, blockSize, minDisparity, maxDisparity, device_)
                          .computeDisparityMapLeft(smoothFactor);
        disparityMapLeft = warp_ ? warpBack(rect, rows_[0], cols_[0]) : rect;
    }
    void computeDisparityMapRight(int blockSize, int minDisparity, int maxDisparity, double smoothFactor,
                                  bool varBlock = false, double thres = 10.0) // default thres: rectification.hpp:66
    {
        MatF64 rect = BlockSearch(left_, right_, blockSize, minDisparity, maxDisparity, device_)
                          .computeDisparityMapRight(smoothFactor, varBlock, thres);
        disparityMapRight = warp_ ? warpBack(rect, rows_[1], cols_[1]) : rect;
    }
    const MatF64 &getDisparityMapLeft() const { return disparityMapLeft; }
    const MatF64 &getDisparityMapRight() const { return disparityMapRight; }

private:
    MatF64 warpBack(const MatF64 &rect, int rows, int cols)
    {
        // H_.inv() by adjugate / determinant, handed on as the warpPerspective matrix
        const double *m = H_;
        const double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
                         m[2] * (m[3] * m[7] - m[4] * m[6]);
        const double r = 1.0 / d;
        const double inv[9] = {(m[4] * m[8] - m[5] * m[7]) * r, (m[2] * m[7] - m[1] * m[8]) * r, (m[1] * m[5] - m[2] * m[4]) * r,
                               (m[5] * m[6] - m[3] * m[8]) * r, (m[0] * m[8] - m[2] * m[6]) * r, (m[2] * m[3] - m[0] * m[5]) * r,
                               (m[3] * m[7] - m[4] * m[6]) * r, (m[1] * m[6] - m[0] * m[7]) * r, (m[0] * m[4] - m[1] * m[3]) * r};
        MatF64 out(rows, cols);
        const int rc = ws_warp_nearest_host(device_.get(), rect.ptr(), rect.cols, rect.rows, rect.cols, inv,
                                            out.ptr(), cols, rows, cols);
        if (rc != WS_OK) throw Error(rc, ws_last_error(device_.get()));
        return out;
    }
    Image8UC3 left_, right_;
    Device &device_;
    double H_[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    int rows_[2] = {0, 0}, cols_[2] = {0, 0};
    bool warp_ = false;
    MatF64 disparityMapLeft, disparityMapRight;
};

// A CV_8UC3 image owned by value (what ImageRectifier::getRectifiedLeft/Right return, rectification.cpp:499-505).
class Mat8UC3 {
public:
    Mat8UC3() = default;
    Mat8UC3(int rows, int cols) : rows(rows), cols(cols), buf_(static_cast<size_t>(rows) * cols * 3, 0) {}
    int rows = 0, cols = 0;
    size_t step() const { return static_cast<size_t>(cols) * 3; }
    uint8_t *ptr() { return buf_.data(); }
    const uint8_t *ptr() const { return buf_.data(); }
    bool empty() const { return buf_.empty(); }
    Image8UC3 view() const { return wsamd::view(buf_.data(), rows, cols); }

private:
    std::vector<uint8_t> buf_;
};

// ImageRectifier (rectification.hpp:50-66) from the point where H_ and Hp_ are known: built from the ORIGINAL pair
// and the two rectifying homographies (the reference estimates them from F and the matches; not on this path).
// Each compute call is one ws_search_unrectified_host: both images rectified on the device
// (warpPerspective(.., H_ / Hp_, size), rectification.cpp:486-493, sizes from ws_rectified_size), the block search,
// and the warp back with H_.inv() to the original size (rectification.cpp:66-88).  The rectified images of the last
// compute call are kept for getRectifiedLeft/Right.  For pairs that are already rectified use RectifiedPair.
class ImageRectifier {
public:
    ImageRectifier(const Image8UC3 &leftImage, const Image8UC3 &rightImage, const double H[9], const double Hp[9],
                   Device &device = Device::shared())
        : leftImage_(leftImage), rightImage_(rightImage), device_(device)
    {
        for (int i = 0; i < 9; ++i) { H_[i] = H[i]; Hp_[i] = Hp[i]; }
        int w, h;
        int rc = ws_rectified_size(H_, leftImage.cols, leftImage.rows, &w, &h);
        if (rc != WS_OK) throw Error(rc, ws_last_error(nullptr));
        leftRectifiedImage_ = Mat8UC3(h, w);
        rc = ws_rectified_size(Hp_, rightImage.cols, rightImage.rows, &w, &h);
        if (rc != WS_OK) throw Error(rc, ws_last_error(nullptr));
        rightRectifiedImage_ = Mat8UC3(h, w);
    }
    void computeDisparityMapLeft(int blockSize, int minDisparity, int maxDisparity, double smoothFactor)
    {
        disparityMapLeft = run(params(WS_VIEW_LEFT, blockSize, minDisparity, maxDisparity, smoothFactor), leftImage_);
    }
    void computeDisparityMapRight(int blockSize, int minDisparity, int maxDisparity, double smoothFactor,
                                  bool varBlock = false, double thres = 10.0) // default thres: rectification.hpp:66
    {
        ws_params p = params(WS_VIEW_RIGHT, blockSize, minDisparity, maxDisparity, smoothFactor);
        p.var_block = varBlock;
        p.thres = thres;
        disparityMapRight = run(p, rightImage_);
    }
    // full size from construction on (ws_rectified_size), all zeros until the first compute call fills them
    const Mat8UC3 &getRectifiedLeft() const { return leftRectifiedImage_; }
    const Mat8UC3 &getRectifiedRight() const { return rightRectifiedImage_; }
    const MatF64 &getDisparityMapLeft() const { return disparityMapLeft; }
    const MatF64 &getDisparityMapRight() const { return disparityMapRight; }
    const double *getH_() const { return H_; }
    const double *getHp_() const { return Hp_; }

    int cost = WS_COST_SSD; // the build's extensions, as on BlockSearch (WS_COST_CENSUS_5X5 / _9X7 included)
    bool subpixel = false;

private:
    ws_params params(int view, int blockSize, int minDisparity, int maxDisparity, double smoothFactor) const
    {
        ws_params p;
        ws_params_default(&p);
        p.view = view;
        p.cost = cost;
        p.block_size = blockSize;
        p.min_disparity = minDisparity;
        p.max_disparity = maxDisparity;
        p.smooth_factor = smoothFactor;
        p.subpixel = subpixel;
        return p;
    }
    MatF64 run(const ws_params &p, const Image8UC3 &frame) // the map comes back in the original frame of `frame`
    {
        MatF64 out(frame.rows, frame.cols);
        const ws_image li = detail::to_c(leftImage_), ri = detail::to_c(rightImage_);
        const int rc = ws_search_unrectified_host(device_.get(), &p, &li, &ri, H_, Hp_, out.ptr(), out.cols, WS_OUT_F64,
                                                  leftRectifiedImage_.ptr(), static_cast<int>(leftRectifiedImage_.step()),
                                                  rightRectifiedImage_.ptr(), static_cast<int>(rightRectifiedImage_.step()));
        if (rc != WS_OK) throw Error(rc, ws_last_error(device_.get()));
        return out;
    }
    Image8UC3 leftImage_, rightImage_;
    Device &device_;
    double H_[9], Hp_[9];
    Mat8UC3 leftRectifiedImage_, rightRectifiedImage_;
    MatF64 disparityMapLeft, disparityMapRight;
};

// A CV_32FC1 map owned by value (what main.cpp:50-64 hands from stage to stage).
class MatF32 {
public:
    MatF32() = default;
    MatF32(int rows, int cols) : rows(rows), cols(cols), buf_(static_cast<size_t>(rows) * cols, 0.0f) {}
    int rows = 0, cols = 0;
    float &at(int y, int x) { return buf_[static_cast<size_t>(y) * cols + x]; }
    float at(int y, int x) const { return buf_[static_cast<size_t>(y) * cols + x]; }
    float *ptr() { return buf_.data(); }
    const float *ptr() const { return buf_.data(); }

private:
    std::vector<float> buf_;
};

// Reconstruction/reconstruction.h:26-33 with the same names and argument order.
inline void removeDisparityOutliers(MatF32 &disparityMap, int kernelSize, float thrFront, float thrBack,
                                    Device &device = Device::shared())
{
    const int rc = ws_remove_disparity_outliers(device.get(), disparityMap.ptr(), disparityMap.cols, disparityMap.rows,
                                                disparityMap.cols, kernelSize, thrFront, thrBack);
    if (rc != WS_OK) throw Error(rc, ws_last_error(device.get()));
}

// Extension: cv::filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) with OpenCV's argument order, on a float32 map in
// place (rules in ws_stereo.h).  In the pipeline it goes after the search (or the left-right check), before
// removeDisparityOutliers and the depth conversion.
inline void filterSpeckles(MatF32 &img, double newVal, int maxSpeckleSize, double maxDiff, Device &device = Device::shared())
{
    ws_speckle_params sp;
    sp.new_val = static_cast<float>(newVal);
    sp.max_speckle_size = maxSpeckleSize;
    sp.max_diff = static_cast<float>(maxDiff);
    const int rc = ws_filter_speckles_host(device.get(), img.ptr(), img.cols, img.rows, img.cols, &sp);
    if (rc != WS_OK) throw Error(rc, ws_last_error(device.get()));
}

// Extension: the census-transform descriptors of an image (rules in ws_stereo.h), row-major, img.cols per row; cost is
// WS_COST_CENSUS_5X5 (24 bits) or WS_COST_CENSUS_9X7 (62 bits).
inline std::vector<uint64_t> censusTransform(const Image8UC3 &img, int cost, Device &device = Device::shared())
{
    std::vector<uint64_t> out(static_cast<size_t>(img.rows > 0 ? img.rows : 0) * static_cast<size_t>(img.cols > 0 ? img.cols : 0));
    const ws_image im = detail::to_c(img);
    const int rc = ws_census_transform_host(device.get(), &im, cost, out.data(), img.cols);
    if (rc != WS_OK) throw Error(rc, ws_last_error(device.get()));
    return out;
}

inline MatF32 convertDisparityToDepth(const MatF32 &dispImage, float focalLength, float baseline,
                                      Device &device = Device::shared())
{
    MatF32 depth(dispImage.rows, dispImage.cols);
    const int rc = ws_convert_disparity_to_depth(device.get(), dispImage.ptr(), dispImage.cols, dispImage.rows,
                                                 dispImage.cols, focalLength, baseline, depth.ptr(), depth.cols);
    if (rc != WS_OK) throw Error(rc, ws_last_error(device.get()));
    return depth;
}

// reconstruction(bgrImage, depthValues, intrinsics, thrMesh) (reconstruction.cpp:152-208); the
// reference's hard-coded output path becomes an argument.  One call (ws_reconstruction_host): the vertices and the
// mesh text are built on the device, only the text comes back to be written.
inline void reconstruction(const Image8UC3 &bgrImage, const MatF32 &depthValues, const float intrinsics[9],
                           float thrMesh, const std::string &meshPath, Device &device = Device::shared())
{
    const ws_image img = detail::to_c(bgrImage);
    const int rc = ws_reconstruction_host(device.get(), depthValues.ptr(), depthValues.cols, depthValues.rows,
                                          depthValues.cols, intrinsics, &img, thrMesh, meshPath.c_str());
    if (rc == WS_ERR_IO) throw Error(rc, "Failed to write mesh! Check file path!");
    if (rc != WS_OK) throw Error(rc, ws_last_error(device.get()));
}

#ifdef WSAMD_WITH_OPENCV
inline Image8UC3 view(const cv::Mat &m)
{
    CV_Assert(m.type() == CV_8UC3);
    return view(m.data, m.rows, m.cols, m.step);
}
inline cv::Mat to_cv(const MatF64 &m)
{
    cv::Mat out(m.rows, m.cols, CV_64F);
    for (int y = 0; y < m.rows; ++y)
        for (int x = 0; x < m.cols; ++x) out.at<double>(y, x) = m.at(y, x);
    return out;
}
#endif

// Many independent pairs over the devices of a node (ws_batch_*): what main.cpp's loop over a dataset becomes when the
// pairs are dealt to several GPUs.  One worker -- a context and a host thread -- per entry of `devices` (a device may
// repeat; empty = every device).  Pairs go whole (longest first, to the least loaded worker) or, where the batch allows
// it, as row bands (bands = true); every map equals BlockSearch's map of that pair.  Not to be shared between threads.
//   wsamd::BatchSearch batch({0, 1, 2, 3, 4, 5, 6, 7});
//   std::vector<wsamd::BatchSearch::Job> jobs;   // {params, left, right} per pair
//   std::vector<wsamd::MatF64> maps = batch.run(jobs);
class BatchSearch {
public:
    struct Job {
        ws_params params;
        Image8UC3 left, right;
    };

    explicit BatchSearch(const std::vector<int> &devices = {})
    {
        ws_batch *b = nullptr;
        const int rc = ws_batch_create(devices.empty() ? nullptr : devices.data(), static_cast<int>(devices.size()), &b);
        if (rc != WS_OK) throw Error(rc, ws_batch_last_error(nullptr));
        batch_.reset(b);
    }
    int workers() const { return ws_batch_workers(batch_.get(), nullptr, 0); }

    // ws_params for one pair: BlockSearch's constructor and method arguments (view = WS_VIEW_LEFT / WS_VIEW_RIGHT)
    static ws_params params(int view, int blockSize, int minDisparity, int maxDisparity, double smoothFactor)
    {
        ws_params p;
        ws_params_default(&p);
        p.view = view;
        p.block_size = blockSize;
        p.min_disparity = minDisparity;
        p.max_disparity = maxDisparity;
        p.smooth_factor = smoothFactor;
        return p;
    }

    // CV_64F maps, one per job, in the order of `jobs`
    std::vector<MatF64> run(const std::vector<Job> &jobs, bool bands = true, int minRows = 256)
    {
        std::vector<MatF64> maps;
        std::vector<ws_job> c(jobs.size());
        maps.reserve(jobs.size());
        for (size_t i = 0; i < jobs.size(); ++i) {
            const Job &j = jobs[i];
            const bool left = j.params.view == WS_VIEW_LEFT;
            maps.emplace_back(left ? j.left.rows : j.right.rows, left ? j.left.cols : j.right.cols);
            c[i] = make_job(j.params, j.left, j.right, maps.back().ptr(), maps.back().cols, WS_OUT_F64);
        }
        run(c, bands, minRows);
        return maps;
    }

    // caller buffers: each ws_job carries its own `out`; every job's status is set.  Throws the first failed job's error.
    void run(std::vector<ws_job> &jobs, bool bands = true, int minRows = 256)
    {
        const int rc = ws_batch_search_host(batch_.get(), jobs.data(), static_cast<int>(jobs.size()), bands ? 1 : 0, minRows);
        if (rc != WS_OK) throw Error(rc, ws_batch_last_error(batch_.get()));
    }

    static ws_job make_job(const ws_params &p, const Image8UC3 &left, const Image8UC3 &right, void *out, int outStride,
                           int outDtype)
    {
        ws_job j;
        j.params = p;
        j.left = detail::to_c(left);
        j.right = detail::to_c(right);
        j.out = out;
        j.out_stride = outStride;
        j.out_dtype = outDtype;
        j.status = WS_JOB_NOT_RUN;
        return j;
    }

#ifdef WSAMD_WITH_OPENCV
    // cv::Mat pairs (CV_8UC3) with one set of parameters: CV_64F maps, written by the library straight into them
    std::vector<cv::Mat> run(const ws_params &p, const std::vector<std::pair<cv::Mat, cv::Mat>> &pairs, bool bands = true,
                             int minRows = 256)
    {
        std::vector<cv::Mat> maps;
        std::vector<ws_job> c;
        maps.reserve(pairs.size());
        for (const auto &pr : pairs) {
            const cv::Mat &size = p.view == WS_VIEW_LEFT ? pr.first : pr.second;
            maps.emplace_back(size.rows, size.cols, CV_64F);
            c.push_back(make_job(p, view(pr.first), view(pr.second), maps.back().data,
                                 static_cast<int>(maps.back().step / sizeof(double)), WS_OUT_F64));
        }
        run(c, bands, minRows);
        return maps;
    }
#endif

private:
    struct Deleter {
        void operator()(ws_batch *b) const { ws_batch_destroy(b); }
    };
    std::unique_ptr<ws_batch, Deleter> batch_;
};

} // namespace wsamd
