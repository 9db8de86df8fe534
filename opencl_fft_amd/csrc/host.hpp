// host.hpp — plumbing shared by the host side of the C ABI (clfft_amd.cpp: FFT plans, pconv_host.cpp, dconv_host.cpp,
// pconv_matrix_host.cpp, nupconv_host.cpp: the convolutions over conv_host.hpp, stft_host.cpp: Stft, pvoc_host.cpp,
// pvoc_frames_host.cpp, pvoc_stream_host.cpp, pvoc_rows_host.cpp, pvoc_signal_host.cpp: Pvoc over pvoc_host.hpp): error
// mapping, device and stream handling, owned device / pinned buffers, numeric switches of the environment, the exact host tables every object needs (the FFT-only ones:
// fft_tables.hpp), the prelude / creation / destruction every object shares, and the staged blocking form of a call
// (staged_call) over the description of its arrays (HostArray; its rules: overlap.hpp).  Each *_host.cpp adds the launch
// headers of its own kernel families (fft_launch.hpp, pconv_launch.hpp, dconv_launch.hpp, stft_launch.hpp, pvoc_launch.hpp,
// tanal_launch.hpp, bank_launch.hpp, pitch_launch.hpp).
// Everything here is inline and hidden (-fvisibility=hidden): nothing becomes an exported symbol.
#pragma once
#include "../../include/clfft_amd.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <utility>
#include <vector>

#include "cpx.hpp"
#include "device_info.hpp"
#include "overlap.hpp"

namespace clfa {

inline constexpr double kPI = 3.141592653589793;  // cl_fft.h:24

inline int map_hip(hipError_t e) {
  switch (e) {
    case hipSuccess: return CLFA_SUCCESS;
    case hipErrorNoDevice: return CLFA_DEVICE_NOT_FOUND;
    case hipErrorInvalidDevice: return CLFA_INVALID_DEVICE;
    case hipErrorOutOfMemory: return CLFA_MEM_OBJECT_ALLOCATION_FAILURE;
    case hipErrorInvalidValue: return CLFA_INVALID_VALUE;
    case hipErrorInvalidDevicePointer: return CLFA_INVALID_MEM_OBJECT;
    case hipErrorInvalidResourceHandle: return CLFA_INVALID_COMMAND_QUEUE;
    case hipErrorNotInitialized:
    case hipErrorInsufficientDriver: return CLFA_DEVICE_NOT_AVAILABLE;
    default: return CLFA_OUT_OF_RESOURCES;
  }
}

#define HIP_TRY(expr)                   \
  do {                                  \
    hipError_t _e = (expr);             \
    if (_e != hipSuccess) {             \
      (void)hipGetLastError();          \
      return map_hip(_e);               \
    }                                   \
  } while (0)

// current-device guard: every entry point works on its object's device and leaves the caller's
// current device as it found it
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t enter(int device) {
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) return e;
    if (prev == device) return hipSuccess;
    e = hipSetDevice(device);
    switched = e == hipSuccess;
    return e;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};
#define ENTER_DEVICE(dev) \
  DeviceGuard _guard;     \
  HIP_TRY(_guard.enter(dev))

// An object owns one device workspace: work on a second stream has to wait for the first.  Switching
// streams is rare (the reference has one queue per object), so the wait is a host-side synchronise
// at the switch instead of an event per launch.
struct StreamOrder {
  hipStream_t last = nullptr;
  bool any = false;
  static bool capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
      (void)hipGetLastError();   // a stale handle: not capturing
      return false;
    }
    return st != hipStreamCaptureStatusNone;
  }
  hipError_t use(hipStream_t s) {
    hipError_t e = hipSuccess;
    if (any && s != last) {
      // a stream under hipGraph capture must not be waited for (nor may anything else be while it
      // captures): captured launches are ordered by the graph, and whatever the object was doing
      // before the capture has to be complete when the graph is replayed — the caller's contract.
      // The same holds when the PREVIOUS stream is the one under capture.
      if (!capturing(s) && !capturing(last)) {
        e = hipStreamSynchronize(last);
        if (e == hipErrorInvalidHandle || e == hipErrorContextIsDestroyed || e == hipErrorInvalidResourceHandle) {
          // the caller has destroyed its previous stream (we do not own it and cannot keep it alive): its handle is
          // gone, its work may not be — wait for the device instead of the handle, and carry on
          (void)hipGetLastError();
          e = hipDeviceSynchronize();
        }
      }
    }
    last = s;
    any = true;
    return e;
  }
};

inline int ilog2(int n) {
  int l = 0;
  while ((1 << l) < n) l++;
  return l;
}
inline bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

// a numeric tuning switch of the environment: atol of its value where that lies strictly between lo and hi, else 0
// (unset, not a number, out of range).  lo >= 0, so 0 never is a value
inline long env_long(const char *name, long lo, long hi) {
  const char *env = getenv(name);
  const long v = env ? atol(env) : 0;
  return v > lo && v < hi ? v : 0;
}

// W_n^k = (cos(2 pi k/n), -sin(2 pi k/n)) rounded from double, the expression of
// cl_fft.cpp:89-90 (`i * 2 * PI / N`) so the float values are bit-identical.
inline void fill_twiddle(std::vector<cpx> &v, int count, int n, int stride, float sign) {
  v.resize(count > 0 ? count : 1);
  for (int i = 0; i < count; i++) {
    int k = i * stride;
    v[i].x = (float)cos(k * 2 * kPI / n);
    v[i].y = sign * (float)sin(k * 2 * kPI / n);
  }
  if (count <= 0) v[0] = mk(1.f, 0.f);
}
// cl_fft.cpp:236-237 (`i * PI / N`)
inline void fill_w2(std::vector<cpx> &v, int m, float sign) {
  v.resize(m);
  for (int i = 0; i < m; i++) {
    v[i].x = (float)cos(i * kPI / m);
    v[i].y = sign * (float)sin(i * kPI / m);
  }
}

// Batches that do not fit a workspace run in chunks.  chunk_items: as many items of `per` bytes as fit `cap` bytes, at
// least one; for_chunks: f(b0, nb) for the chunks [b0, b0 + nb) of `batch` items, at most `chunk` each, until one fails
inline long chunk_items(size_t per, size_t cap) { return cap / per > 0 ? (long)(cap / per) : 1; }
template <class F>
inline int for_chunks(long batch, long chunk, F f) {
  for (long b0 = 0; b0 < batch; b0 += chunk)
    if (int e = f(b0, batch - b0 < chunk ? batch - b0 : chunk)) return e;
  return 0;
}

// Device memory owned by an object, freed with it (on the current device: destroy functions delete their object while
// the object's device is current).  Objects hold these by value and are never copied.
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  int ensure(size_t want) {
    if (want <= bytes) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return map_hip(e);
    }
    bytes = want;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  void swap(DevBuf &o) {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
  }
};

// pinned host memory mapped into the device's address space: kernels read / write it directly over
// PCIe.  For the few KiB of one audio block that beats three hipMemcpyAsync calls (10-15 us each).
struct HostBuf {
  void *h = nullptr;   // host pointer
  void *d = nullptr;   // the same memory as the device sees it
  size_t bytes = 0;
  HostBuf() = default;
  HostBuf(const HostBuf &) = delete;
  HostBuf &operator=(const HostBuf &) = delete;
  ~HostBuf() { release(); }
  int ensure(size_t want) {
    if (want <= bytes) return 0;
    release();
    hipError_t e = hipHostMalloc(&h, want, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&d, h, 0);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      release();
      return map_hip(e);
    }
    bytes = want;
    return 0;
  }
  void release() {
    if (h) (void)hipHostFree(h);
    h = d = nullptr;
    bytes = 0;
  }
};

inline int upload(DevBuf &b, const void *src, size_t bytes) {
  int e = b.ensure(bytes);
  if (e) return e;
  HIP_TRY(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}
// the tables of an n-point packed real transform: W_n^k, k < n / 2 (forward sign), and the pair table of `sign`
inline int upload_half(DevBuf &b, int n) {
  std::vector<cpx> h;
  fill_twiddle(h, n / 2, n, 1, -1.f);
  return upload(b, h.data(), sizeof(cpx) * h.size());
}
inline int upload_w2(DevBuf &b, int n, float sign) {
  std::vector<cpx> h;
  fill_w2(h, n, sign);
  return upload(b, h.data(), sizeof(cpx) * n);
}

inline int device_info(int device, DeviceInfo &di) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    return CLFA_DEVICE_NOT_FOUND;
  }
  if (device < 0 || device >= count) return CLFA_INVALID_DEVICE;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  di.device = device;
  di.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  return 0;
}

// the prelude of an entry point: a NULL object is an invalid value, an object whose creation failed returns that error
//   if (int e = obj_error(p)) return e;
template <class T>
inline int obj_error(const T *p) {
  return !p ? CLFA_INVALID_VALUE : p->err;
}

// every *_create: allocate, set up (the object keeps the setup's code as its error), hand the object out either way
template <class T, class Setup>
inline int create_object(T **out, Setup setup) {
  if (!out) return CLFA_INVALID_VALUE;
  T *p = new (std::nothrow) T();
  if (!p) return CLFA_OUT_OF_HOST_MEMORY;
  p->err = setup(p);
  *out = p;
  return p->err;
}

// every *_destroy: on the object's device, drain and destroy its stream, run `extra` (what the object owns besides its
// buffers), then delete it — its DevBuf / HostBuf members free themselves while that device is still current
template <class T, class Extra>
inline void destroy_object(T *p, Extra extra) {
  if (!p) return;
  DeviceGuard guard;
  (void)guard.enter(p->di.device);
  if (p->stream) {
    (void)hipStreamSynchronize(p->stream);
    (void)hipStreamDestroy(p->stream);
  }
  extra(p);
  delete p;
}
template <class T>
inline void destroy_object(T *p) {
  destroy_object(p, [](T *) {});
}

// workspaces that the first call needing them allocates: refused while the stream is captured (a hipMalloc there would
// be outside the graph).  A want of 0 bytes is never missing.
struct Want {
  DevBuf *b;
  size_t bytes;
};
inline int ensure_workspaces(std::initializer_list<Want> want, hipStream_t s) {
  bool missing = false;
  for (const Want &w : want) missing = missing || w.b->bytes < w.bytes;
  if (!missing) return CLFA_SUCCESS;
  if (StreamOrder::capturing(s)) return CLFA_INVALID_OPERATION;
  for (const Want &w : want) {
    int e = w.b->ensure(w.bytes);
    if (e) return e;
  }
  return CLFA_SUCCESS;
}

// One array of a call of the object T (CallArray, overlap.hpp) with where a blocking form stages it: a DevBuf member of
// T, the rows packed there; HostArrays: the list a function that describes a call's arrays returns
template <class T>
using HostArray = CallArray<DevBuf T::*>;
template <class T, size_t N>
struct HostArrays {
  HostArray<T> a[N];
};
constexpr size_t kCallArrays = 5;   // at most so many per call

// The blocking form around a device form, on the object's device (the caller has entered it): every array the call looks
// at has its staging buffer, ensured in the order of the list; the inputs are copied in (strided rows packed), dev(d) runs
// the device work on the staged arrays d[i] (NULL where the call does not look) and the object's stream, every output is
// copied out (to the caller's strided rows), and the stream is waited for, once.  A staging buffer holds one array of a
// call: a list whose used arrays name one buffer twice is an invalid operation.
template <class T, size_t N, class Dev>
inline int staged_call(T *p, const HostArray<T> (&arrays)[N], Dev dev) {
  static_assert(N <= kCallArrays, "kCallArrays");
  for (size_t i = 0; i < N; i++)
    for (size_t k = 0; k < i; k++)
      if (arrays[i].used && arrays[k].used && arrays[i].stage == arrays[k].stage) return CLFA_INVALID_OPERATION;
  const void *d[kCallArrays] = {};
  for (size_t i = 0; i < N; i++) {
    const HostArray<T> &a = arrays[i];
    if (int e = a.used ? (p->*a.stage).ensure(a.bytes * a.rows) : 0) return e;
    if (a.used) d[i] = (p->*a.stage).p;
  }
  const auto copy = [&](size_t i) {   // between the caller's rows and the packed staging, the way the array goes
    const HostArray<T> &a = arrays[i];
    void *dst = const_cast<void *>(a.out ? a.ptr : d[i]);
    const void *src = a.out ? d[i] : a.ptr;
    const hipMemcpyKind kind = a.out ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
    if (!a.pitch) return hipMemcpyAsync(dst, src, a.bytes * a.rows, kind, p->stream);
    return hipMemcpy2DAsync(dst, a.out ? a.pitch : a.bytes, src, a.out ? a.bytes : a.pitch, a.bytes, a.rows, kind, p->stream);
  };
  for (size_t i = 0; i < N; i++)
    if (d[i] && !arrays[i].out) HIP_TRY(copy(i));
  if (int e = dev(d)) return e;
  for (size_t i = 0; i < N; i++)
    if (d[i] && arrays[i].out) HIP_TRY(copy(i));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return CLFA_SUCCESS;
}

}  // namespace clfa
