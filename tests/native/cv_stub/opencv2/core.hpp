// Minimal stand-in for <opencv2/core.hpp>: only what include/vslam_adapter.hpp uses under -DVSLAM_WITH_OPENCV, with the
// shapes OpenCV 4 gives them (type = depth + ((channels - 1) << 3); Mat::step a MatStep that converts to size_t; a Mat
// built on caller data does not own it, an allocated one is reference-counted).  Test-only: lets the shim's OpenCV branch
// compile and run where OpenCV is not installed.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#define CV_CN_SHIFT 3
#define CV_DEPTH_MAX (1 << CV_CN_SHIFT)
#define CV_MAT_DEPTH_MASK (CV_DEPTH_MAX - 1)
#define CV_MAT_DEPTH(flags) ((flags) & CV_MAT_DEPTH_MASK)
#define CV_MAKETYPE(depth, cn) (CV_MAT_DEPTH(depth) + (((cn) - 1) << CV_CN_SHIFT))
#define CV_MAT_CN(flags) ((((flags) >> CV_CN_SHIFT) & 511) + 1)
#define CV_8U 0
#define CV_8S 1
#define CV_16U 2
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_8UC2 CV_MAKETYPE(CV_8U, 2)
#define CV_8UC3 CV_MAKETYPE(CV_8U, 3)
#define CV_8UC4 CV_MAKETYPE(CV_8U, 4)
#define CV_8UC(n) CV_MAKETYPE(CV_8U, (n))

namespace cv {

typedef unsigned char uchar;

static inline size_t elem_size1(int depth) { return depth <= CV_8S ? 1 : depth <= 3 ? 2 : depth <= 5 ? 4 : 8; }

struct MatStep {
    size_t buf[2] = {0, 0};
    operator size_t() const { return buf[0]; }
    size_t operator[](int i) const { return buf[i]; }
};

template <typename T> struct Point_ {
    T x{}, y{};
    Point_() {}
    Point_(T x_, T y_) : x(x_), y(y_) {}
};
typedef Point_<float> Point2f;

class KeyPoint {
  public:
    KeyPoint() {}
    KeyPoint(float x, float y, float size_, float angle_ = -1, float response_ = 0, int octave_ = 0, int class_id_ = -1)
        : pt(x, y), size(size_), angle(angle_), response(response_), octave(octave_), class_id(class_id_) {}
    Point2f pt;
    float size{0}, angle{-1}, response{0};
    int octave{0}, class_id{-1};
};

class Mat {
  public:
    static const size_t AUTO_STEP = 0;
    Mat() {}
    Mat(int rows_, int cols_, int type) { create(rows_, cols_, type); }
    Mat(int rows_, int cols_, int type, void* data_, size_t step_ = AUTO_STEP) : rows(rows_), cols(cols_), flags(type) {
        data = (uchar*)data_;
        step.buf[0] = step_ == AUTO_STEP ? (size_t)cols_ * elemSize() : step_;
        step.buf[1] = elemSize();
    }
    void create(int rows_, int cols_, int type) {
        rows = rows_; cols = cols_; flags = type;
        step.buf[0] = (size_t)cols_ * elemSize(); step.buf[1] = elemSize();
        store_ = std::make_shared<std::vector<uchar>>(step.buf[0] * (size_t)rows_);
        data = store_->data();
    }
    int type() const { return flags; }
    int depth() const { return CV_MAT_DEPTH(flags); }
    int channels() const { return CV_MAT_CN(flags); }
    size_t elemSize() const { return elem_size1(depth()) * (size_t)channels(); }
    bool empty() const { return data == nullptr; }
    template <typename T = uchar> T* ptr(int row = 0) { return (T*)(data + (size_t)row * step.buf[0]); }
    template <typename T = uchar> const T* ptr(int row = 0) const { return (const T*)(data + (size_t)row * step.buf[0]); }

    int rows = 0, cols = 0;
    uchar* data = nullptr;
    MatStep step;

  private:
    int flags = 0;
    std::shared_ptr<std::vector<uchar>> store_;
};

}  // namespace cv
