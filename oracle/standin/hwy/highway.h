// oracle/standin/hwy/highway.h -- TEST INFRASTRUCTURE ONLY.
//
// A scalar stand-in for the part of the Google Highway API the reference's adapter and sequence code calls, written from
// the API's documented meaning so that those translation units compile unmodified without the library.  Every vector has
// a fixed 16 lanes held in a plain array; every operation is a loop over the lanes.  Semantics that decide results:
//   LoadN(d, p, n)   loads min(n, 16) lanes and sets the lanes past n to zero (and reads nothing past p + n);
//   StoreN(v, d, p, n) writes only the first min(n, 16) lanes;
//   SlideDownLanes(d, v, k): lane i takes lane i + k, the top k lanes become zero;
//   Reverse(d, v):   lane i takes lane 15 - i.
#pragma once
#include <cstddef>
#include <cstdint>

#define HWY_NAMESPACE N_SCALAR16
#define HWY_BEFORE_NAMESPACE() static_assert(true, "")
#define HWY_AFTER_NAMESPACE() static_assert(true, "")
#define HWY_RESTRICT __restrict__
#define HWY_ATTR
#define HWY_UNLIKELY(x) __builtin_expect(!!(x), 0)
#define HWY_DASSERT(x) \
    do {               \
    } while (0)

namespace hwy {
namespace HWY_NAMESPACE {

constexpr size_t kStandInLanes = 16;

template <typename T>
struct Simd {
    using T_ = T;
};
template <typename T>
using ScalableTag = Simd<T>;
template <class D>
using TFromD = typename D::T_;

template <typename T>
struct Vec16 {
    T raw[kStandInLanes];
};
template <typename T>
struct Mask16 {
    bool raw[kStandInLanes];
};
template <class D>
using Vec = Vec16<TFromD<D>>;
template <class D>
using Mask = Mask16<TFromD<D>>;

template <class D>
constexpr size_t Lanes(D) {
    return kStandInLanes;
}

template <class D>
Vec<D> Set(D, TFromD<D> x) {
    Vec<D> v;
    for (size_t i = 0; i < kStandInLanes; i++) v.raw[i] = x;
    return v;
}

template <class D>
Vec<D> LoadU(D, const TFromD<D>* HWY_RESTRICT p) {
    Vec<D> v;
    for (size_t i = 0; i < kStandInLanes; i++) v.raw[i] = p[i];
    return v;
}
template <class D>
Vec<D> LoadN(D, const TFromD<D>* HWY_RESTRICT p, size_t n) {
    Vec<D> v;
    for (size_t i = 0; i < kStandInLanes; i++) v.raw[i] = i < n ? p[i] : TFromD<D>(0);
    return v;
}
template <class D>
void StoreU(const Vec<D>& v, D, TFromD<D>* HWY_RESTRICT p) {
    for (size_t i = 0; i < kStandInLanes; i++) p[i] = v.raw[i];
}
template <class D>
void StoreN(const Vec<D>& v, D, TFromD<D>* HWY_RESTRICT p, size_t n) {
    for (size_t i = 0; i < kStandInLanes && i < n; i++) p[i] = v.raw[i];
}

template <typename T>
Mask16<T> operator!=(const Vec16<T>& a, const Vec16<T>& b) {
    Mask16<T> m;
    for (size_t i = 0; i < kStandInLanes; i++) m.raw[i] = a.raw[i] != b.raw[i];
    return m;
}
template <typename T>
Mask16<T> Eq(const Vec16<T>& a, const Vec16<T>& b) {
    Mask16<T> m;
    for (size_t i = 0; i < kStandInLanes; i++) m.raw[i] = a.raw[i] == b.raw[i];
    return m;
}
template <typename T>
Mask16<T> Or(const Mask16<T>& a, const Mask16<T>& b) {
    Mask16<T> m;
    for (size_t i = 0; i < kStandInLanes; i++) m.raw[i] = a.raw[i] || b.raw[i];
    return m;
}
template <typename T>
Vec16<T> IfThenElse(const Mask16<T>& m, const Vec16<T>& yes, const Vec16<T>& no) {
    Vec16<T> v;
    for (size_t i = 0; i < kStandInLanes; i++) v.raw[i] = m.raw[i] ? yes.raw[i] : no.raw[i];
    return v;
}
template <class D>
size_t CountTrue(D, const Mask<D>& m) {
    size_t n = 0;
    for (size_t i = 0; i < kStandInLanes; i++) n += m.raw[i] ? 1 : 0;
    return n;
}
template <class D>
Vec<D> Reverse(D, const Vec<D>& v) {
    Vec<D> r;
    for (size_t i = 0; i < kStandInLanes; i++) r.raw[i] = v.raw[kStandInLanes - 1 - i];
    return r;
}
template <class D>
Vec<D> SlideDownLanes(D, const Vec<D>& v, size_t k) {
    Vec<D> r;
    for (size_t i = 0; i < kStandInLanes; i++) r.raw[i] = i + k < kStandInLanes ? v.raw[i + k] : TFromD<D>(0);
    return r;
}

}  // namespace HWY_NAMESPACE
}  // namespace hwy
