// io_fields.hpp -- the argument blocks of the optional stages of the C ABI (object filter, rigid bodies, marker tracker, body tracker) and
// the ONE list of each block's arrays: every layout, staging copy and copy-back of a stage goes through these lists, so a
// field's type and element count are written once.  No HIP here: tests/native/io_fields_check.cpp compiles this for the host.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

// Sub-buffers of one allocation, each padded to `align` bytes.  A layout is ONE function that takes its fields from a
// Carver and returns `off`: run on a null base it gives the size to reserve, run on the buffer it gives the pointers.
struct Carver {
  uintptr_t base;
  size_t align, off = 0;
  explicit Carver(void* b, size_t align_ = 256) : base((uintptr_t)b), align(align_) {}
  template <class T>
  static size_t padded(size_t count, size_t align = 256) { return (sizeof(T) * count + align - 1) / align * align; }
  template <class T>
  T* take(size_t count) {
    T* p = (T*)(base + off);
    off += padded<T>(count, align);
    return p;
  }
  void align_to(size_t a) { off = (off + a - 1) / a * a; }
};

// what the element counts are made of: frames, points per frame (K_max), body slots per frame (B_max), filtered objects
struct IoDims {
  size_t F, K = 0, B = 0, D = 0;
};

// Each list calls fn(member, element count) once per array, in the order of the C ABI.  A member that points to const is an
// input of the stage (its time stamps); every other one is an output.
// object filter over the locator's outputs (object_filter_capi.hip); every pointer device-accessible
struct FilterIO {
  const double* t;  // [F]
  float* fpos;      // [F][D][3]
  float* fvel;      // [F][D][3]
  double* fheading; // [F][D]
  int32_t* chosen;  // [F][D]
  template <class Fn>
  static void fields(const IoDims& n, Fn&& fn) {
    fn(&FilterIO::t, n.F);
    fn(&FilterIO::fpos, n.F * n.D * 3);
    fn(&FilterIO::fvel, n.F * n.D * 3);
    fn(&FilterIO::fheading, n.F * n.D);
    fn(&FilterIO::chosen, n.F * n.D);
  }
};
// rigid bodies over the frame path's points (rigid_body_capi.hip); every pointer device-accessible, arrays [F][B_max]
struct BodiesIO {
  int B_max;        // body slots per frame (>= the registered bodies; the slots beyond them are zero-filled)
  int32_t* found;
  int32_t* n_used;
  int8_t* assign;   // [F][B_max][8]
  double* R;        // [F][B_max][9]
  double* t;        // [F][B_max][3]
  double* rms;
  double* score;
  int32_t* status;
  static constexpr size_t kAssign = 8;  // (MOCAP_RB_MAX_MARKERS: rigid_body_capi.hip asserts it)
  template <class Fn>
  static void fields(const IoDims& n, Fn&& fn) {
    const size_t FB = n.F * n.B;
    fn(&BodiesIO::found, FB);
    fn(&BodiesIO::n_used, FB);
    fn(&BodiesIO::assign, FB * kAssign);
    fn(&BodiesIO::R, FB * 9);
    fn(&BodiesIO::t, FB * 3);
    fn(&BodiesIO::rms, FB);
    fn(&BodiesIO::score, FB);
    fn(&BodiesIO::status, FB);
  }
};
// marker tracker over the frame path's points (marker_track_capi.hip); every pointer device-accessible
struct MarkersIO {
  const double* t;    // [F]
  int32_t* id;        // [F][K_max]
  int32_t* hits;      // [F][K_max]
  int32_t* n_tracks;  // [F]
  int32_t* status;    // [F]
  template <class Fn>
  static void fields(const IoDims& n, Fn&& fn) {
    fn(&MarkersIO::t, n.F);
    fn(&MarkersIO::id, n.F * n.K);
    fn(&MarkersIO::hits, n.F * n.K);
    fn(&MarkersIO::n_tracks, n.F);
    fn(&MarkersIO::status, n.F);
  }
};
// body tracker behind the rigid bodies (body_track_capi.hip); every pointer device-accessible, arrays [F][B_max] but t, status
struct TrackedIO {
  const double* t;    // [F] time stamps
  int32_t* tracked;
  int32_t* source;
  int32_t* n_used;
  int8_t* assign;     // [F][B_max][8]
  double* R;          // [F][B_max][9]
  double* p;          // [F][B_max][3]: the pose's translation (the t of BodiesIO)
  double* rms;
  int32_t* hits;
  int32_t* missed;
  int32_t* status;    // [F]
  template <class Fn>
  static void fields(const IoDims& n, Fn&& fn) {
    const size_t FB = n.F * n.B;
    fn(&TrackedIO::t, n.F);
    fn(&TrackedIO::tracked, FB);
    fn(&TrackedIO::source, FB);
    fn(&TrackedIO::n_used, FB);
    fn(&TrackedIO::assign, FB * BodiesIO::kAssign);
    fn(&TrackedIO::R, FB * 9);
    fn(&TrackedIO::p, FB * 3);
    fn(&TrackedIO::rms, FB);
    fn(&TrackedIO::hits, FB);
    fn(&TrackedIO::missed, FB);
    fn(&TrackedIO::status, n.F);
  }
};

// every array of `io`, inputs included, out of the carver
template <class IO>
void carve(Carver& c, IO& io, const IoDims& n) {
  IO::fields(n, [&](auto m, size_t count) {
    using T = std::remove_const_t<std::remove_pointer_t<std::remove_reference_t<decltype(io.*m)>>>;
    io.*m = c.take<T>(count);
  });
}

// The inputs (kInputs) or the outputs of `src` into the same arrays of `dst`, through copy(dst, src, bytes) -> 0 or an error
// code: memcpy between the pinned block and the caller's arrays, hipMemcpyAsync (StreamCopy, ctx.hpp) for the staged entry
// points.  Arrays of no elements are left alone (their pointers may be null); the first error ends the copying.
struct HostCopy {
  int operator()(void* dst, const void* src, size_t bytes) const { return memcpy(dst, src, bytes), 0; }
};
template <bool kInputs, class IO, class Copy>
int copy_fields(const IO& dst, const IO& src, const IoDims& n, Copy&& copy) {
  int rc = 0;
  IO::fields(n, [&](auto m, size_t count) {
    using T = std::remove_pointer_t<std::remove_reference_t<decltype(src.*m)>>;
    if (std::is_const_v<T> == kInputs && count && !rc) rc = copy((void*)(dst.*m), (const void*)(src.*m), sizeof(T) * count);
  });
  return rc;
}
