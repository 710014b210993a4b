// hsflow.hpp -- header-only C++ host layer over the C ABI (hsflow.h),
// OpenCV-free.  Mirrors the reference's operator class
// HornSchunckOF/hornSchunck.cpp:8-76 on plain image views:
//
//   hsflow::HornSchunck hs(windowSize, maxIterations, alpha);   // :13-17
//   hs.getGradients(prev, next, gx, gy, gt);                      // :19-41
//   hs.getFlow(prev, next, u, v);                                  // :43-75
//
// Same public fields, same argument meaning, outputs float64 row-major
// (what CV_64FC1 holds).  Errors throw hsflow::Error (the reference throws
// cv::Exception from inside OpenCV).  Copies share one device context, so a
// copy-initialised object (main.cpp:97) reuses the cached device buffers.
// Link: -lhsflow (cpp-optical-flow_amd/libhsflow.so).
#pragma once

#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "hsflow.h"

namespace hsflow {

class Error : public std::runtime_error {
  public:
    Error(int status, const std::string &msg)
        : std::runtime_error("hsflow: " + msg + " (" + hsflow_status_string(status) + ")"),
          status_(status) {}
    int status() const { return status_; }

  private:
    int status_;
};

// One single-channel image: U8 (CV_8UC1), F32 (CV_32FC1) or F64 (CV_64FC1);
// `step` = bytes between rows (cv::Mat::step), so ROIs need no copy.
struct ImageView {
    const void *data = nullptr;
    int rows = 0, cols = 0;
    size_t step = 0;
    int type = HSFLOW_U8;
};

inline ImageView view(const uint8_t *p, int rows, int cols, size_t step = 0) {
    return {p, rows, cols, step ? step : (size_t)cols, HSFLOW_U8};
}
inline ImageView view(const float *p, int rows, int cols, size_t step = 0) {
    return {p, rows, cols, step ? step : (size_t)cols * 4, HSFLOW_F32};
}
inline ImageView view(const double *p, int rows, int cols, size_t step = 0) {
    return {p, rows, cols, step ? step : (size_t)cols * 8, HSFLOW_F64};
}

// One decoded 8-bit colour frame, interleaved BGR (CV_8UC3, what cv::imread
// returns); `step` = bytes between rows, 0 = dense (3 * cols).
struct BgrView {
    const uint8_t *data = nullptr;
    int rows = 0, cols = 0;
    size_t step = 0;
};

// What the interpolating calls do with a pair whose flows fail the
// forward-backward check (hsflow.h, "fallback for a failed pair"): mode
// HSFLOW_FALLBACK_NEAREST or HSFLOW_FALLBACK_BLEND, and the share of consistent
// pixels below which a pair fails.
struct Fallback : hsflow_fallback {
    Fallback(int mode = HSFLOW_FALLBACK_NEAREST, float min_share = HSFLOW_FALLBACK_MIN_SHARE)
        : hsflow_fallback{mode, min_share} {}
};

// RAII device context (device, stream, cached buffers).
class Context {
  public:
    explicit Context(int device = 0) {
        int rc = hsflow_create(&ctx_, device);
        if (rc != HSFLOW_OK) throw Error(rc, hsflow_last_error(nullptr));
    }
    ~Context() { hsflow_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    hsflow_ctx *get() const { return ctx_; }
    void check(int rc) const {
        if (rc != HSFLOW_OK) throw Error(rc, hsflow_last_error(ctx_));
    }
    // The brightness-robust prefilter (hsflow.h, hsflow_ctx_set_prefilter) the
    // warped, bidirectional and interpolating solves run on the frames first;
    // nullptr or mode 0 = off (default).  getFlow and getGradients ignore it.
    void setPrefilter(const hsflow_prefilter *pf) { check(hsflow_ctx_set_prefilter(ctx_, pf)); }
    hsflow_prefilter prefilter() const {
        hsflow_prefilter pf{};
        check(hsflow_ctx_prefilter(ctx_, &pf));
        return pf;
    }
    // The smoothness term of the same solves (hsflow.h, hsflow_ctx_set_smoothness):
    // HSFLOW_SMOOTH_FLOW_DRIVEN weights each tap of the window mean by a
    // diffusivity of the current flow, which keeps motion boundaries sharp;
    // nullptr or mode 0 = quadratic (default).  windowSize must then be 3 or 5.
    void setSmoothness(const hsflow_smoothness *sm) { check(hsflow_ctx_set_smoothness(ctx_, sm)); }
    hsflow_smoothness smoothness() const {
        hsflow_smoothness sm{};
        check(hsflow_ctx_smoothness(ctx_, &sm));
        return sm;
    }
    // Sequence mode (hsflow.h, hsflow_ctx_set_temporal): the bidirectional and
    // interpolating solves start from the flow predicted from the previous such
    // call and leave a prediction for the next; feed them the consecutive
    // pairs of one clip.  Keep `levels` and halve `warps` when motion may
    // change, levels = 1 only for steady motion, resetTemporal() at a scene
    // cut.  Off by default.
    void setTemporal(bool on) { check(hsflow_ctx_set_temporal(ctx_, on ? 1 : 0)); }
    bool temporal() const {
        const int rc = hsflow_ctx_temporal(ctx_);
        if (rc < 0) check(rc);
        return rc != 0;
    }
    void resetTemporal() { check(hsflow_ctx_temporal_reset(ctx_)); }
    // The last pyramid level the same solves solve (hsflow.h,
    // hsflow_ctx_set_finest_level): finest > 0 stops the solve at that level
    // and brings its flow to the full frame bilinearly; frames are still
    // interpolated at full resolution.  Must be < the call's levels.  0, the
    // default: the full frame.
    void setFinestLevel(int finest) { check(hsflow_ctx_set_finest_level(ctx_, finest)); }
    int finestLevel() const {
        const int rc = hsflow_ctx_finest_level(ctx_);
        if (rc < 0) check(rc);
        return rc;
    }
    // Flow projection for the interpolating calls (hsflow.h,
    // hsflow_ctx_set_projection): 1 carries both flows to each time before
    // the blend, so a pixel near a motion boundary takes the flow of the
    // surface that lands on it; 0, the default: the flows at the pixel itself.
    void setProjection(int projection) { check(hsflow_ctx_set_projection(ctx_, projection)); }
    int projection() const {
        const int rc = hsflow_ctx_projection(ctx_);
        if (rc < 0) check(rc);
        return rc;
    }
    // The fallback of the interpolating calls (hsflow.h, hsflow_ctx_set_fallback):
    // a pair whose flows fail the check -- a scene cut, a motion beyond the
    // pyramid's reach -- comes back as a source frame or a cross-fade; nullptr
    // or mode 0 = off (default).  lastCut: the last such call's verdict, 1 for
    // a cut, 0 for a pair that passed, -1 where there was none.
    void setFallback(const hsflow_fallback *fb) { check(hsflow_ctx_set_fallback(ctx_, fb)); }
    Fallback fallback() const {
        Fallback fb(HSFLOW_FALLBACK_OFF, 0.0f);
        check(hsflow_ctx_fallback(ctx_, &fb));
        return fb;
    }
    int lastCut() const { return hsflow_ctx_last_cut(ctx_); }

    // The packed 4:2:0 frames at `times` between two packed 8-bit 4:2:0 frames
    // of `layout` (HSFLOW_YUV_I420 or HSFLOW_YUV_NV12), rows * cols * 3 / 2 bytes
    // each, rows and cols the luma's and even (hsflow.h, hsflow_flow_interp_yuv):
    // the solve runs on the luma planes as they are, the chroma follows the same
    // flows on its own grid; no colour conversion.  frames[k]: the frame at
    // times[k] in the same layout; flags[k]: rows * cols HSFLOW_INTERP_* bytes,
    // the luma's.  The context's prefilter, smoothness, finest level, sequence
    // mode and fallback apply, lastCut() is set.  projection -1: none, and on
    // a context with the projection on the call throws; 0 or 1: that, whatever
    // the context's setting (hsflow_flow_interp_yuv_pj: the chroma reads its
    // time-t flow through the luma's winners).
    void getFrameInterpYuv(const uint8_t *prev, const uint8_t *next, int layout, int rows,
                           int cols, const std::vector<float> &times, int levels, int warps,
                           int median, int windowSize, int maxIterations, double alpha,
                           std::vector<std::vector<uint8_t>> &frames,
                           std::vector<std::vector<uint8_t>> *flags = nullptr,
                           int projection = -1) {
        if (!prev || !next) throw Error(HSFLOW_ERR_ARG, "empty image");
        if (rows < 2 || cols < 2 || rows % 2 || cols % 2)
            throw Error(HSFLOW_ERR_ARG, "YUV 4:2:0 needs even rows and cols");
        const size_t n = (size_t)rows * cols;
        frames.resize(times.size());
        if (flags) flags->resize(times.size());
        std::vector<void *> out(times.size());
        std::vector<uint8_t *> fl(times.size());
        for (size_t k = 0; k < times.size(); ++k) {
            frames[k].resize(n / 2 * 3);
            out[k] = frames[k].data();
            if (flags) (*flags)[k].resize(n), fl[k] = (*flags)[k].data();
        }
        if (projection < 0) {
            check(hsflow_flow_interp_yuv(ctx_, prev, next, layout, rows, cols, levels, warps,
                                         median, windowSize, maxIterations, alpha,
                                         HSFLOW_CONSISTENCY_REL, HSFLOW_CONSISTENCY_ABS,
                                         times.data(), (int)times.size(), out.data(), HSFLOW_U8,
                                         flags ? fl.data() : nullptr, nullptr));
            return;
        }
        check(hsflow_flow_interp_yuv_pj(ctx_, prev, next, layout, rows, cols, levels, warps,
                                        median, windowSize, maxIterations, alpha,
                                        HSFLOW_CONSISTENCY_REL, HSFLOW_CONSISTENCY_ABS,
                                        times.data(), (int)times.size(), projection, out.data(),
                                        HSFLOW_U8, flags ? fl.data() : nullptr, nullptr));
    }

    // The same for packed frames of rows * cols * 3 / 2 16-bit samples each
    // (yuv420p10le .. p16le: HSFLOW_YUV_I420; P010 .. P016: HSFLOW_YUV_NV12), in
    // and out (hsflow.h, hsflow_flow_interp_yuv16).  A sample is its value, so
    // alpha scales with the content: x 4 for 10-bit LSB-aligned samples, x 256
    // for P010, relative to 8-bit.  projection 0 or 1; -1 stands for 0: the
    // context's projection setting is not consulted.
    void getFrameInterpYuv(const uint16_t *prev, const uint16_t *next, int layout, int rows,
                           int cols, const std::vector<float> &times, int levels, int warps,
                           int median, int windowSize, int maxIterations, double alpha,
                           std::vector<std::vector<uint16_t>> &frames,
                           std::vector<std::vector<uint8_t>> *flags = nullptr,
                           int projection = -1) {
        if (!prev || !next) throw Error(HSFLOW_ERR_ARG, "empty image");
        if (rows < 2 || cols < 2 || rows % 2 || cols % 2)
            throw Error(HSFLOW_ERR_ARG, "YUV 4:2:0 needs even rows and cols");
        const size_t n = (size_t)rows * cols;
        frames.resize(times.size());
        if (flags) flags->resize(times.size());
        std::vector<void *> out(times.size());
        std::vector<uint8_t *> fl(times.size());
        for (size_t k = 0; k < times.size(); ++k) {
            frames[k].resize(n / 2 * 3);
            out[k] = frames[k].data();
            if (flags) (*flags)[k].resize(n), fl[k] = (*flags)[k].data();
        }
        check(hsflow_flow_interp_yuv16(ctx_, prev, next, layout, rows, cols, levels, warps,
                                       median, windowSize, maxIterations, alpha,
                                       HSFLOW_CONSISTENCY_REL, HSFLOW_CONSISTENCY_ABS,
                                       times.data(), (int)times.size(),
                                       projection < 0 ? 0 : projection, out.data(), HSFLOW_U16,
                                       flags ? fl.data() : nullptr, nullptr));
    }

  private:
    hsflow_ctx *ctx_ = nullptr;
};

// `pf` on a context for one call (nullptr: the context's own setting stays)
class PrefilterScope {
  public:
    PrefilterScope(Context &c, const hsflow_prefilter *pf) : c_(c), on_(pf != nullptr) {
        if (!on_) return;
        was_ = c_.prefilter();
        c_.setPrefilter(pf);
    }
    ~PrefilterScope() {
        if (on_) hsflow_ctx_set_prefilter(c_.get(), &was_);
    }
    PrefilterScope(const PrefilterScope &) = delete;
    PrefilterScope &operator=(const PrefilterScope &) = delete;

  private:
    Context &c_;
    bool on_;
    hsflow_prefilter was_{};
};

class HornSchunck {
  public:
    // hornSchunck.cpp:10-11 -- public, same names
    int windowSize, maxIterations;
    double alpha;

    // hornSchunck.cpp:13-17
    HornSchunck(int inpWindowSize, int inpMaxIterations, double inpAlpha, int device = 0)
        : windowSize(inpWindowSize), maxIterations(inpMaxIterations), alpha(inpAlpha),
          device_(device) {}

    // hornSchunck.cpp:19-41 -> Ix, Iy, It as rows*cols float64
    void getGradients(const ImageView &imagePrev, const ImageView &imageNext,
                      std::vector<double> &gradX, std::vector<double> &gradY,
                      std::vector<double> &gradT) {
        check_pair(imagePrev, imageNext);
        const size_t n = (size_t)imagePrev.rows * imagePrev.cols;
        gradX.resize(n);
        gradY.resize(n);
        gradT.resize(n);
        getGradientsInto(imagePrev, imageNext, gradX.data(), gradY.data(), gradT.data(),
                         HSFLOW_F64, (size_t)imagePrev.cols * 8);
    }

    // hornSchunck.cpp:43-75 -> u, v as rows*cols float64 (reallocated, like
    // the reference's u = cv::Mat::zeros(...) at :49-50)
    void getFlow(const ImageView &imagePrev, const ImageView &imageNext,
                 std::vector<double> &u, std::vector<double> &v) {
        check_pair(imagePrev, imageNext);
        const size_t n = (size_t)imagePrev.rows * imagePrev.cols;
        u.resize(n);
        v.resize(n);
        getFlowInto(imagePrev, imageNext, u.data(), v.data(), HSFLOW_F64,
                    (size_t)imagePrev.cols * 8);
    }

    // Warped coarse-to-fine solve for motions beyond a pixel (hsflow.h,
    // hsflow_flow_warped): `levels` pyramid levels, per level `warps`
    // re-linearisations around the current flow with maxIterations
    // iterations each.  u, v as getFlow; 8 (u, v) is the motion in pixels.
    // median = 3 or 5: a median x median filter of (u, v) after every warp's
    // iterations (hsflow_flow_warped_median), which makes alpha ~ 100 usable
    // and keeps a moving object's edges; 0 = none.  prefilter: the solve runs
    // on the locally normalised frames (hsflow.h, hsflow_prefilter; exposure
    // steps, fades, flicker), set on the context for this call; nullptr
    // leaves the context's own setting (setPrefilter; off by default).
    void setPrefilter(const hsflow_prefilter *pf) { ctx().setPrefilter(pf); }
    // the flow-driven smoothness term for the same methods (Context::setSmoothness)
    void setSmoothness(const hsflow_smoothness *sm) { ctx().setSmoothness(sm); }
    // sequence mode for getFlowBidir, getFrameInterp and getFrameInterpBgr
    // (Context::setTemporal); getFlowWarped has no backward flow and ignores it
    void setTemporal(bool on) { ctx().setTemporal(on); }
    bool temporal() { return ctx().temporal(); }
    void resetTemporal() { ctx().resetTemporal(); }
    // the last pyramid level the same methods solve (Context::setFinestLevel)
    void setFinestLevel(int finest) { ctx().setFinestLevel(finest); }
    int finestLevel() { return ctx().finestLevel(); }
    // flow projection for getFrameInterp and getFrameInterpBgr
    // (Context::setProjection)
    void setProjection(int projection) { ctx().setProjection(projection); }
    int projection() { return ctx().projection(); }
    // the fallback for a failed pair of getFrameInterp and getFrameInterpBgr
    // (Context::setFallback), and the last call's verdict
    void setFallback(const hsflow_fallback *fb) { ctx().setFallback(fb); }
    Fallback fallback() { return ctx().fallback(); }
    int lastCut() { return ctx().lastCut(); }
    void getFlowWarped(const ImageView &imagePrev, const ImageView &imageNext, int levels,
                       int warps, std::vector<double> &u, std::vector<double> &v,
                       int median = 0, const hsflow_prefilter *prefilter = nullptr) {
        check_pair(imagePrev, imageNext);
        const size_t n = (size_t)imagePrev.rows * imagePrev.cols;
        u.resize(n);
        v.resize(n);
        std::vector<double> ha, hb;
        const ImageView a = common_type(imagePrev, imageNext, ha);
        const ImageView b = common_type(imageNext, imagePrev, hb);
        Context &c = ctx();
        PrefilterScope scope(c, prefilter);
        c.check(hsflow_flow_warped_median(c.get(), a.data, b.data, a.type, a.rows, a.cols, a.step,
                                          b.step, levels, warps, median, windowSize,
                                          maxIterations, alpha, u.data(), v.data(), HSFLOW_F64,
                                          (size_t)a.cols * 8));
    }

    // getFlowWarped plus where its answer can be trusted (hsflow.h,
    // hsflow_flow_bidir): the solve also runs next -> prev, and `mask` gets
    // the forward check per pixel -- HSFLOW_CONSISTENT, HSFLOW_INCONSISTENT or
    // HSFLOW_OUT_OF_FRAME -- at the default thresholds.  median as in
    // and prefilter as in getFlowWarped, for both directions.
    void getFlowBidir(const ImageView &imagePrev, const ImageView &imageNext, int levels,
                      int warps, std::vector<double> &u, std::vector<double> &v,
                      std::vector<uint8_t> &mask, int median = 0,
                      const hsflow_prefilter *prefilter = nullptr) {
        check_pair(imagePrev, imageNext);
        const size_t n = (size_t)imagePrev.rows * imagePrev.cols;
        u.resize(n);
        v.resize(n);
        mask.resize(n);
        std::vector<double> ha, hb;
        const ImageView a = common_type(imagePrev, imageNext, ha);
        const ImageView b = common_type(imageNext, imagePrev, hb);
        Context &c = ctx();
        PrefilterScope scope(c, prefilter);
        c.check(hsflow_flow_bidir_median(
            c.get(), a.data, b.data, a.type, a.rows, a.cols, a.step, b.step, levels, warps, median,
            windowSize, maxIterations, alpha, HSFLOW_CONSISTENCY_REL, HSFLOW_CONSISTENCY_ABS,
            u.data(), v.data(), nullptr, nullptr, HSFLOW_F64, (size_t)a.cols * 8, mask.data(),
            nullptr, (size_t)a.cols, nullptr));
    }

    // The frames at `times` (each in [0, 1], at most HSFLOW_MAX_TIMES) between
    // imagePrev (t = 0) and imageNext (t = 1): getFlowBidir's solve, then the
    // motion-compensated blend (hsflow.h, hsflow_flow_interp).  planes[k]: the
    // frame at times[k] as rows*cols float32 grey levels; flags[k]: per pixel
    // the HSFLOW_INTERP_* bits, 0 where both source pixels pass the
    // forward-backward check at the default thresholds.  prefilter as in
    // getFlowWarped: the flows come from the prefiltered frames, the frames
    // themselves are sampled.
    void getFrameInterp(const ImageView &imagePrev, const ImageView &imageNext,
                        const std::vector<float> &times, int levels, int warps, int median,
                        std::vector<std::vector<float>> &planes,
                        std::vector<std::vector<uint8_t>> *flags = nullptr,
                        const hsflow_prefilter *prefilter = nullptr) {
        check_pair(imagePrev, imageNext);
        const size_t n = (size_t)imagePrev.rows * imagePrev.cols;
        planes.resize(times.size());
        if (flags) flags->resize(times.size());
        std::vector<void *> out(times.size());
        std::vector<uint8_t *> fl(times.size());
        for (size_t k = 0; k < times.size(); ++k) {
            planes[k].resize(n);
            out[k] = planes[k].data();
            if (flags) (*flags)[k].resize(n), fl[k] = (*flags)[k].data();
        }
        std::vector<double> ha, hb;
        const ImageView a = common_type(imagePrev, imageNext, ha);
        const ImageView b = common_type(imageNext, imagePrev, hb);
        Context &c = ctx();
        PrefilterScope scope(c, prefilter);
        c.check(hsflow_flow_interp(
            c.get(), a.data, b.data, a.type, a.rows, a.cols, a.step, b.step, levels, warps, median,
            windowSize, maxIterations, alpha, HSFLOW_CONSISTENCY_REL, HSFLOW_CONSISTENCY_ABS,
            times.data(), (int)times.size(), out.data(), HSFLOW_F32, (size_t)a.cols * 4,
            flags ? fl.data() : nullptr, (size_t)a.cols, nullptr));
    }
    void getFrameInterp(const ImageView &imagePrev, const ImageView &imageNext,
                        const std::vector<float> &times, int levels, int warps, int median,
                        std::vector<std::vector<float>> &planes,
                        std::vector<std::vector<uint8_t>> &flags,
                        const hsflow_prefilter *prefilter = nullptr) {
        getFrameInterp(imagePrev, imageNext, times, levels, warps, median, planes, &flags,
                       prefilter);
    }

    // getFrameInterp for colour frames (hsflow.h, hsflow_flow_interp_bgr): the
    // frames go up as BGR, the solve runs on their grey conversion, and each
    // channel gets the motion-compensated blend.  frames[k]: the frame at
    // times[k] as rows*cols*3 uint8, interleaved BGR; flags[k]: rows*cols
    // HSFLOW_INTERP_* bytes, one per pixel.  prefilter as in getFlowWarped, run
    // on the grey planes.
    void getFrameInterpBgr(const BgrView &prev, const BgrView &next,
                           const std::vector<float> &times, int levels, int warps, int median,
                           std::vector<std::vector<uint8_t>> &frames,
                           std::vector<std::vector<uint8_t>> *flags = nullptr,
                           const hsflow_prefilter *prefilter = nullptr) {
        if (!prev.data || !next.data) throw Error(HSFLOW_ERR_ARG, "empty image");
        if (prev.rows != next.rows || prev.cols != next.cols)
            throw Error(HSFLOW_ERR_SIZE, "Image sizes are different");
        const size_t n = (size_t)prev.rows * prev.cols;
        frames.resize(times.size());
        if (flags) flags->resize(times.size());
        std::vector<void *> out(times.size());
        std::vector<uint8_t *> fl(times.size());
        for (size_t k = 0; k < times.size(); ++k) {
            frames[k].resize(n * 3);
            out[k] = frames[k].data();
            if (flags) (*flags)[k].resize(n), fl[k] = (*flags)[k].data();
        }
        const size_t dense = (size_t)prev.cols * 3;
        Context &c = ctx();
        PrefilterScope scope(c, prefilter);
        c.check(hsflow_flow_interp_bgr(
            c.get(), prev.data, next.data, prev.rows, prev.cols, prev.step ? prev.step : dense,
            next.step ? next.step : dense, levels, warps, median, windowSize, maxIterations,
            alpha, HSFLOW_CONSISTENCY_REL, HSFLOW_CONSISTENCY_ABS, times.data(),
            (int)times.size(), out.data(), HSFLOW_U8, dense, flags ? fl.data() : nullptr,
            (size_t)prev.cols, nullptr));
    }

    // getFrameInterp for packed 8-bit 4:2:0 frames (Context::getFrameInterpYuv,
    // with this object's window, iterations and alpha)
    void getFrameInterpYuv(const uint8_t *prev, const uint8_t *next, int layout, int rows,
                           int cols, const std::vector<float> &times, int levels, int warps,
                           int median, std::vector<std::vector<uint8_t>> &frames,
                           std::vector<std::vector<uint8_t>> *flags = nullptr,
                           int projection = -1) {
        ctx().getFrameInterpYuv(prev, next, layout, rows, cols, times, levels, warps, median,
                                windowSize, maxIterations, alpha, frames, flags, projection);
    }
    // ... and for packed frames of 16-bit samples
    void getFrameInterpYuv(const uint16_t *prev, const uint16_t *next, int layout, int rows,
                           int cols, const std::vector<float> &times, int levels, int warps,
                           int median, std::vector<std::vector<uint16_t>> &frames,
                           std::vector<std::vector<uint8_t>> *flags = nullptr,
                           int projection = -1) {
        ctx().getFrameInterpYuv(prev, next, layout, rows, cols, times, levels, warps, median,
                                windowSize, maxIterations, alpha, frames, flags, projection);
    }

    // Raw form for callers that own output rows (cv::Mat adapter): dtype_out
    // HSFLOW_F64 or HSFLOW_F32, out_step in bytes.  Each frame keeps its own
    // row step; frames of different element types are both widened to
    // float64 first, as hornSchunck.cpp:23-24 converts each with convertTo.
    void getFlowInto(const ImageView &imagePrev, const ImageView &imageNext, void *u,
                     void *v, int dtype_out, size_t out_step) {
        check_pair(imagePrev, imageNext);
        std::vector<double> ha, hb;
        const ImageView a = common_type(imagePrev, imageNext, ha);
        const ImageView b = common_type(imageNext, imagePrev, hb);
        Context &c = ctx();
        c.check(hsflow_flow(c.get(), a.data, b.data, a.type, a.rows, a.cols, a.step, b.step,
                            windowSize, maxIterations, alpha, u, v, dtype_out, out_step));
    }
    void getGradientsInto(const ImageView &imagePrev, const ImageView &imageNext, void *gx,
                          void *gy, void *gt, int dtype_out, size_t out_step) {
        check_pair(imagePrev, imageNext);
        std::vector<double> ha, hb;
        const ImageView a = common_type(imagePrev, imageNext, ha);
        const ImageView b = common_type(imageNext, imagePrev, hb);
        Context &c = ctx();
        c.check(hsflow_gradients(c.get(), a.data, b.data, a.type, a.rows, a.cols, a.step,
                                 b.step, gx, gy, gt, dtype_out, out_step));
    }

  private:
    int device_;
    std::shared_ptr<Context> ctx_;

    Context &ctx() {
        if (!ctx_) ctx_ = std::make_shared<Context>(device_);
        return *ctx_;
    }
    static void check_pair(const ImageView &a, const ImageView &b) {
        if (!a.data || !b.data) throw Error(HSFLOW_ERR_ARG, "empty image");
        if (a.rows != b.rows || a.cols != b.cols)
            throw Error(HSFLOW_ERR_SIZE, "Image sizes are different");
    }
    static double half_to_double(uint16_t h) {  // IEEE binary16 (CV_16F)
        const int e = (h >> 10) & 31, f = h & 1023;
        const double s = (h & 0x8000) ? -1.0 : 1.0;
        if (e == 0) return s * std::ldexp((double)f, -24);
        if (e == 31) return f ? std::nan("") : s * HUGE_VAL;
        return s * std::ldexp((double)(f | 1024), e - 25);
    }
    // `m` as it enters the ABI: unchanged when both frames share an element
    // type, else widened to a dense float64 copy held in `hold`.
    static ImageView common_type(const ImageView &m, const ImageView &other,
                                 std::vector<double> &hold) {
        if (m.type == other.type) return m;
        hold.resize((size_t)m.rows * m.cols);
        for (int r = 0; r < m.rows; ++r) {
            const char *row = (const char *)m.data + (size_t)r * m.step;
            double *d = hold.data() + (size_t)r * m.cols;
            for (int c = 0; c < m.cols; ++c) {
                switch (m.type) {
                case HSFLOW_U8: d[c] = ((const uint8_t *)row)[c]; break;
                case HSFLOW_F32: d[c] = ((const float *)row)[c]; break;
                case HSFLOW_F64: d[c] = ((const double *)row)[c]; break;
                case HSFLOW_F16: d[c] = half_to_double(((const uint16_t *)row)[c]); break;
                default: throw Error(HSFLOW_ERR_ARG, "unsupported element type");
                }
            }
        }
        return {hold.data(), m.rows, m.cols, (size_t)m.cols * 8, HSFLOW_F64};
    }
};

// compute(I0, I1, alpha, nIter) -> (u, v): the north-star convenience form.
inline void compute(const ImageView &I0, const ImageView &I1, double alpha, int nIter,
                    std::vector<double> &u, std::vector<double> &v, int windowSize = 5) {
    HornSchunck(windowSize, nIter, alpha).getFlow(I0, I1, u, v);
}

// Frame-parallel getFlow over several GPUs from one process
// (hsflow_flow_multi): pair j (prev[j], next[j], all one size, type and row
// steps) on devices[j % devices.size()]; u[j], v[j] receive CV_64FC1-style
// rows x cols doubles (resized here).
inline void flowMulti(const std::vector<int> &devices, const std::vector<ImageView> &prev,
                      const std::vector<ImageView> &next, int windowSize, int maxIterations,
                      double alpha, std::vector<std::vector<double>> &u,
                      std::vector<std::vector<double>> &v) {
    if (prev.size() != next.size()) throw Error(HSFLOW_ERR_ARG, "prev/next counts differ");
    const size_t n = prev.size();
    u.resize(n);
    v.resize(n);
    if (n == 0) return;
    const ImageView &a = prev[0], &b = next[0];
    std::vector<const void *> I0(n), I1(n);
    std::vector<void *> pu(n), pv(n);
    for (size_t j = 0; j < n; ++j) {
        if (prev[j].rows != a.rows || prev[j].cols != a.cols || prev[j].type != a.type ||
            prev[j].step != a.step || next[j].rows != a.rows || next[j].cols != a.cols ||
            next[j].type != a.type || next[j].step != b.step)
            throw Error(HSFLOW_ERR_SIZE, "pairs differ in size, type or row step");
        I0[j] = prev[j].data;
        I1[j] = next[j].data;
        u[j].assign((size_t)a.rows * a.cols, 0.0);
        v[j].assign((size_t)a.rows * a.cols, 0.0);
        pu[j] = u[j].data();
        pv[j] = v[j].data();
    }
    const int rc = hsflow_flow_multi(devices.data(), (int)devices.size(), (int)n, I0.data(),
                                     I1.data(), a.type, a.rows, a.cols, a.step, b.step,
                                     windowSize, maxIterations, alpha, pu.data(), pv.data(),
                                     HSFLOW_F64, (size_t)a.cols * sizeof(double));
    if (rc != HSFLOW_OK) throw Error(rc, hsflow_last_error(nullptr));
}

}  // namespace hsflow
