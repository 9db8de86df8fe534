// clfft_amd.cpp — C ABI of libclfft_amd.so (see include/clfft_amd.h): library, devices, error strings, tables, copy
// helpers and the FFT plans.  The convolutions are in pconv_host.cpp, dconv_host.cpp, pconv_matrix_host.cpp and
// nupconv_host.cpp, Stft in stft_host.cpp, what they share in host.hpp.
//
// Host side of the hot path: plan objects (the reference's Clcfft / Clrfft instances), exact host tables, H2D/D2H
// staging for the blocking host-pointer entry points, and the mapping hipError_t -> OpenCL status numbers.  No CPU
// compute fallback exists: without a HIP device every constructor reports CL_DEVICE_NOT_FOUND and every exec call fails.
#include <utility>

#include "fft_launch.hpp"
#include "fft_route.hpp"
#include "fft_tables.hpp"
#include "host.hpp"

using namespace clfa;

// ---------------------------------------------------------------------------------
// plan objects
// ---------------------------------------------------------------------------------

struct clfa_fft {
  DeviceInfo di;
  FftShape sh;           // what fft_route() decides by (fft_route.hpp); sh.n = complex length (Clrfft: M = size/2, cl_fft.cpp:210)
  int size = 0;          // user-visible size (n, or real points for Clrfft)
  int err = 0;           // Clcfft::cl_err
  char log[2048];
  hipStream_t stream = nullptr;
  DevBuf half, w2, four, scratch, stage, res16;
  DevBuf own1, own2;     // the reference's protected data1 / data2 (cl_fft.h:35), on request: clfa_fft_device_buffers
  DevBuf own_w, own_b;   // ... and w / b: clfa_fft_device_tables
  bool own_tables_ready = false;   // both tables allocated AND filled
  struct Pinned {          // a pinned array the caller got from the plan: clfa_fft_host_alloc
    char *h, *d;           // host address, and the same memory as the device sees it
    size_t bytes;
  };
  std::vector<Pinned> pinned;
  clfa_fft *own_cplx = nullptr;    // Clrfft::fft() = the complex n-point transform alone (cl_fft.cpp:138-151 on N = size / 2): a c2c plan, on demand
  StreamOrder order;
  HostBuf zstage;        // zero-copy staging of small host transforms
  FftTables tabs;
  // n > 65536 (extension): n = N1 x N2; `tabs` then belongs to the N2-point row transform
  BigGeom big{};
  DevBuf bigtabs, scratch2;
  // complex n = 65536: the resident kernel's counters (kRes16CtrBytes behind the workspace, a guard line on either side:
  // zeroed once at creation, left zero by every launch) and, on request, its per-workgroup records (clfa_fft_balance_record)
  unsigned *res16_ctr = nullptr;
  bool res16_static = false;   // CLFA_RES16_STATIC=1 (a measuring switch, read at creation): the static assignment always
  DevBuf res16_rec;
  int rec_grid = 0;        // workgroups of the last recorded launch
  // any other length (extension): Bluestein around two power-of-two plans of length sh.blue_m
  clfa_fft *blue_f = nullptr, *blue_i = nullptr;
  DevBuf blue_w, blue_b, blue_work;
};

extern "C" {

// ---------------------------------------------------------------------------------
// library / devices
// ---------------------------------------------------------------------------------

const char *clfa_version(void) { return "clfft_amd 0.1 (gfx950)"; }

int clfa_device_count(int *count) {
  if (!count) return CLFA_INVALID_VALUE;
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess || c <= 0) {
    (void)hipGetLastError();
    *count = 0;
    return CLFA_DEVICE_NOT_FOUND;
  }
  *count = c;
  return CLFA_SUCCESS;
}

int clfa_device_name(int device, char *buf, size_t len) {
  if (!buf || len == 0) return CLFA_INVALID_VALUE;
  DeviceInfo di;
  int e = device_info(device, di);
  if (e) return e;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  const char *nm = prop.name[0] ? prop.name : prop.gcnArchName;
  snprintf(buf, len, "%s", nm);
  return CLFA_SUCCESS;
}

// message table of cl_fft::cl_error_string (cl_fft.cpp:298-395)
const char *clfa_error_string(int err) {
  static const struct {
    int code;
    const char *msg;
  } tab[] = {{0, "Success!"}, {-1, "Device not found."}, {-2, "Device not available"},
             {-3, "Compiler not available"}, {-4, "Memory object allocation failure"},
             {-5, "Out of resources"}, {-6, "Out of host memory"},
             {-7, "Profiling information not available"}, {-8, "Memory copy overlap"},
             {-9, "Image format mismatch"}, {-10, "Image format not supported"},
             {-11, "Program build failure"}, {-12, "Map failure"}, {-30, "Invalid value"},
             {-31, "Invalid device type"}, {-32, "Invalid platform"}, {-33, "Invalid device"},
             {-34, "Invalid context"}, {-35, "Invalid queue properties"}, {-36, "Invalid command queue"},
             {-37, "Invalid host pointer"}, {-38, "Invalid memory object"},
             {-39, "Invalid image format descriptor"}, {-40, "Invalid image size"},
             {-41, "Invalid sampler"}, {-42, "Invalid binary"}, {-43, "Invalid build options"},
             {-44, "Invalid program"}, {-45, "Invalid program executable"}, {-46, "Invalid kernel name"},
             {-47, "Invalid kernel definition"}, {-48, "Invalid kernel"}, {-49, "Invalid argument index"},
             {-50, "Invalid argument value"}, {-51, "Invalid argument size"},
             {-52, "Invalid kernel arguments"}, {-53, "Invalid work dimension"},
             {-54, "Invalid work group size"}, {-55, "Invalid work item size"},
             {-56, "Invalid global offset"}, {-57, "Invalid event wait list"}, {-58, "Invalid event"},
             {-59, "Invalid operation"}, {-60, "Invalid OpenGL object"}, {-61, "Invalid buffer size"},
             {-62, "Invalid mip-map level"}};
  for (const auto &t : tab)
    if (t.code == err) return t.msg;
  return "Unknown error";
}

// ---------------------------------------------------------------------------------
// tables
// ---------------------------------------------------------------------------------

int clfa_bitrev_table(int n, int *out) {
  if (!out || !is_pow2(n)) return CLFA_INVALID_VALUE;
  // doubling construction of cl_fft.cpp:96-101
  out[0] = 0;
  for (int i = 1, h = n / 2; i < n; i <<= 1, h >>= 1)
    for (int j = 0; j < i; j++) out[i + j] = out[j] + h;
  return CLFA_SUCCESS;
}

int clfa_twiddle_table(int n, int forward, float *out) {
  if (!out || n < 1) return CLFA_INVALID_VALUE;
  std::vector<cpx> v;
  fill_twiddle(v, n, n, 1, forward ? -1.f : 1.f);
  memcpy(out, v.data(), sizeof(cpx) * n);
  return CLFA_SUCCESS;
}

int clfa_r2c_twiddle_table(int m, int forward, float *out) {
  if (!out || m < 1) return CLFA_INVALID_VALUE;
  std::vector<cpx> v;
  fill_w2(v, m, forward ? -1.f : 1.f);
  memcpy(out, v.data(), sizeof(cpx) * m);
  return CLFA_SUCCESS;
}

// ---------------------------------------------------------------------------------
// FFT plans
// ---------------------------------------------------------------------------------

// host double-precision radix-2 transform (unscaled, forward sign), for the Bluestein filter table
static void host_fft(std::vector<double> &re, std::vector<double> &im) {
  const size_t n = re.size();
  for (size_t i = 1, j = 0; i < n; i++) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) {
      std::swap(re[i], re[j]);
      std::swap(im[i], im[j]);
    }
  }
  for (size_t len = 2; len <= n; len <<= 1) {
    const size_t h = len / 2;
    std::vector<double> c(h), sn(h);
    for (size_t k = 0; k < h; k++) {
      c[k] = cos(2 * kPI * (double)k / (double)len);
      sn[k] = -sin(2 * kPI * (double)k / (double)len);
    }
    for (size_t i = 0; i < n; i += len)
      for (size_t k = 0; k < h; k++) {
        const double xr = re[i + k + h] * c[k] - im[i + k + h] * sn[k], xi = re[i + k + h] * sn[k] + im[i + k + h] * c[k];
        re[i + k + h] = re[i + k] - xr;
        im[i + k + h] = im[i + k] - xi;
        re[i + k] += xr;
        im[i + k] += xi;
      }
  }
}

// any length that is not a power of two (extension): chirp w[j] = exp(-+ i pi j^2 / n) (j^2 reduced mod 2 n
// in integers, then double), filter B = DFT_m(conj(w) wrapped round m) in double, two m-point sub-plans
static int blue_setup(clfa_fft *p, int n, bool fwd) {
  const int device = p->di.device, m = p->sh.blue_m;
  int e;
  const double sgn = fwd ? -1.0 : 1.0;
  std::vector<cpx> w(n), bt(m);
  std::vector<double> br(m, 0.0), bi(m, 0.0);
  for (int j = 0; j < n; j++) {
    const long long q = ((long long)j * j) % (2LL * n);
    const double a = kPI * (double)q / (double)n;
    w[j] = mk((float)cos(a), (float)(sgn * sin(a)));
    br[j] = cos(a);
    bi[j] = -sgn * sin(a);              // conj(w)
    if (j) {
      br[m - j] = br[j];
      bi[m - j] = bi[j];
    }
  }
  host_fft(br, bi);
  for (int k = 0; k < m; k++) bt[k] = mk((float)br[k], (float)bi[k]);
  if ((e = upload(p->blue_w, w.data(), sizeof(cpx) * n))) return e;
  if ((e = upload(p->blue_b, bt.data(), sizeof(cpx) * m))) return e;
  if ((e = clfa_cfft_create(&p->blue_f, device, m, 1))) return e;
  if ((e = clfa_cfft_create(&p->blue_i, device, m, 0))) return e;
  // workspace: as many m-point rows as fit 256 MiB; exec walks the batch in such chunks (k_blue_lds: one launch, none)
  if (fft_route_many(p->sh) == FftRoute::Bluestein) return p->blue_work.ensure(sizeof(cpx) * (size_t)m * chunk_items(sizeof(cpx) * (size_t)m, (size_t)256 << 20));
  return CLFA_SUCCESS;
}

// Whatever the routes the shape can ever take need (fft_needs): a plan carries the tables of all of them and exec picks by
// batch.  n > 65536: the big-N tables and chunk workspace here, the rest for the row transform, its workspace in scratch2.
static int fft_setup(clfa_fft *p, int device, int n, bool real, int size, bool fwd) {
  p->sh.real = real;
  p->sh.fwd = fwd;
  p->sh.n = n;
  p->size = size;
  p->log[0] = 0;
  if (n < 2 || (is_pow2(n) && n > (1 << kBigMaxLog)) || (!is_pow2(n) && n > kBlueMaxN)) {
    snprintf(p->log, sizeof(p->log), "complex length must be 2..%d (powers of two) or 2..%d (other lengths), got %d",
             1 << kBigMaxLog, kBlueMaxN, n);
    return CLFA_INVALID_VALUE;
  }
  if (!is_pow2(n) && real && (n & 1)) {
    snprintf(p->log, sizeof(p->log), "real sizes that are not powers of two must be multiples of 4 (got %d)", 2 * n);
    return CLFA_INVALID_VALUE;
  }
  int e = device_info(device, p->di);
  if (e) return e;
  p->sh = fft_shape(real, fwd, n, p->di.num_cus);
  ENTER_DEVICE(device);
  HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  if (real) {
    if ((e = upload_w2(p->w2, n, fwd ? -1.f : 1.f))) return e;
    p->tabs.w2 = (const cpx *)p->w2.p;
  }
  if (p->sh.blue_m) return blue_setup(p, n, fwd);
  std::vector<cpx> h;
  FftShape rows = p->sh;   // the transform the LDS / four-step tables are for
  if (fft_needs(p->sh) & kNeedBig) {
    big_split(p->sh.logn, &p->big);
    rows = fft_shape(false, fwd, 1 << p->big.logn2, p->sh.num_cus);
    fill_big_tables(h, n, 1 << p->big.logn1);
    if ((e = upload(p->bigtabs, h.data(), sizeof(cpx) * h.size()))) return e;
    // workspace: as many whole transforms as fit 256 MiB (at least one); exec walks the batch in such chunks
    const long mb = env_long("CLFA_BIG_CHUNK_MB", 0, 1L << 31);   // tuning switch, read once
    const size_t per = sizeof(cpx) * (size_t)n;
    if ((e = p->scratch.ensure(per * chunk_items(per, (size_t)(mb ? mb : 256) << 20)))) return e;
  }
  const unsigned needs = fft_needs(rows);
  auto put = [&](DevBuf &b, const cpx *&tab) {
    const int err = upload(b, h.data(), sizeof(cpx) * h.size());
    tab = (const cpx *)b.p;
    return err;
  };
  if (needs & (kNeedHalf | kNeedHalf2x)) {
    if (needs & kNeedHalf2x) fill_lane_tables(h, rows.logn - 1, rows.logn == 14);
    else if (kLdsTwoLevel(rows.logn)) fill_lane_tables(h, rows.logn, false);
    else fill_twiddle(h, rows.n / 2, rows.n, 1, -1.f);
    if ((e = put(p->half, p->tabs.half))) return e;
  }
  if (needs & kNeedFour) fill_fourstep_tables(h, rows.logn);
  if ((needs & kNeedFour) && (e = put(p->four, p->tabs.four))) return e;
  if (needs & kNeedRes16) fill_res16_tables(h);
  if ((needs & kNeedRes16) && (e = put(p->res16, p->tabs.res16))) return e;
  DevBuf &ws = rows.logn == p->sh.logn ? p->scratch : p->scratch2;
  if (!(needs & kNeedFourWs)) return CLFA_SUCCESS;
  const size_t wsb = (size_t)fourstep_grid(p->di) * rows.n * sizeof(cpx);
  // the plan's own complex n = 65536 transform: the shared assignment's counters behind the workspace proper (whose first
  // part are the slots; the few-transform route writes up to num_cus / 4 transforms there, so the counters follow its
  // end), between two guard lines.  The packed real size-131072 plans run the static assignment: no counters.
  const bool ctr = !real && (needs & kNeedRes16) && rows.logn == p->sh.logn;
  if ((e = ws.ensure(wsb + (ctr ? kRes16CtrBytes + 2 * kRes16GuardBytes : 0)))) return e;
  if (ctr) {
    char *g = (char *)ws.p + wsb;
    p->res16_ctr = (unsigned *)(g + kRes16GuardBytes);
    HIP_TRY(hipMemsetAsync(g, (int)(kRes16GuardWord & 0xff), kRes16CtrBytes + 2 * kRes16GuardBytes, p->stream));
    HIP_TRY(hipMemsetAsync(p->res16_ctr, 0, kRes16CtrBytes, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));   // launches may follow on any stream
    p->res16_static = env_long("CLFA_RES16_STATIC", 0, 2) != 0;
  }
  return CLFA_SUCCESS;
}

int clfa_cfft_create(clfa_fft **plan, int device, int n, int forward) {
  return create_object(plan, [&](clfa_fft *p) { return fft_setup(p, device, n, false, n, forward != 0); });
}

int clfa_rfft_create(clfa_fft **plan, int device, int size, int forward) {
  return create_object(plan, [&](clfa_fft *p) {
    if (size < 4 || (size & 1)) {
      snprintf(p->log, sizeof(p->log), "real size must be even, 4..%d (got %d)", 2 << kBigMaxLog, size);
      return CLFA_INVALID_VALUE;
    }
    return fft_setup(p, device, size / 2, true, size, forward != 0);
  });
}

void clfa_fft_destroy(clfa_fft *p) {
  destroy_object(p, [](clfa_fft *q) {
    for (auto &r : q->pinned) (void)hipHostFree(r.h);
    q->pinned.clear();
    if (q->own_cplx) clfa_fft_destroy(q->own_cplx);
    if (q->blue_f) clfa_fft_destroy(q->blue_f);
    if (q->blue_i) clfa_fft_destroy(q->blue_i);
  });
}

int clfa_fft_get_error(const clfa_fft *p) { return p ? p->err : CLFA_INVALID_VALUE; }
const char *clfa_fft_get_log(const clfa_fft *p) { return p ? p->log : ""; }
size_t clfa_fft_workspace_bytes(const clfa_fft *p) {
  if (!p) return 0;
  size_t sub = p->blue_f ? clfa_fft_workspace_bytes(p->blue_f) + clfa_fft_workspace_bytes(p->blue_i) : 0;
  return p->scratch.bytes + p->scratch2.bytes + p->blue_work.bytes + sub;
}

// the kernel of a batch above every threshold
const char *clfa_fft_kernel_name(const clfa_fft *p) { return p ? route_kernel_name(fft_route_many(p->sh), p->sh) : ""; }

static int fft_exec(clfa_fft *p, cpx *d, long off, long batch, hipStream_t s);

// FftRoute::Bluestein: src -> dst, the batch in chunks of the workspace's rows
static int blue_exec(clfa_fft *p, const cpx *src, cpx *dst, long batch, hipStream_t s) {
  const int n = p->sh.n, m = p->sh.blue_m;
  cpx *work = (cpx *)p->blue_work.p;
  const cpx *w = (const cpx *)p->blue_w.p, *bt = (const cpx *)p->blue_b.p;
  return for_chunks(batch, (long)(p->blue_work.bytes / (sizeof(cpx) * (size_t)m)), [&](long b0, long nb) -> int {
    HIP_TRY(launch_blue_pre(src + b0 * (long)n, w, work, n, m, nb, s));
    int e = fft_exec(p->blue_f, work, 0, nb, s);
    if (e) return e;
    HIP_TRY(launch_blue_mul(work, bt, m, nb, s));
    if ((e = fft_exec(p->blue_i, work, 0, nb, s))) return e;
    HIP_TRY(launch_blue_post(work, w, dst + b0 * (long)n, n, m, p->sh.fwd ? 1.0f / (float)n : 1.0f, nb, s));
    return CLFA_SUCCESS;
  });
}

// The body of every device-resident transform: `d` is read, the results go to d + off complex elements (off = 0: in
// place; otherwise a destination that does not overlap the source, which is then left untouched).  Two-pass routes run
// their FIRST pass from the source to the destination and the rest in place there.
static int fft_exec(clfa_fft *p, cpx *d, long off, long batch, hipStream_t s) {
  const FftShape &sh = p->sh;
  const bool fwd = sh.fwd, scale = sh.fwd;  // cl_fft.cpp:39-40: forward plans divide by N, inverse plans do not
  const FftRoute route = fft_route(sh, batch);
  // real plans on a route of the complex transform: the reference's pack / unpack as a pass of its own; the unpack lands
  // in the destination, where the transform then runs in place
  const bool apart = sh.real && route_pack_apart(route);
  cpx *o = d + off, *scratch = (cpx *)p->scratch.p;
  if (apart && !fwd) {
    HIP_TRY(launch_c2r_unpack(d, p->tabs.w2, sh.n, batch, s, off));
    d = o;
  }
  switch (route) {
    case FftRoute::Lds: HIP_TRY(launch_fft_lds(sh.logn, fwd, fft_mode(sh), scale, d, p->tabs, batch, p->di, s, off)); break;
    case FftRoute::Cfft2x13: HIP_TRY(launch_cfft_2x13(fwd, scale, d, p->tabs, batch, p->di, s, off)); break;
    case FftRoute::Rfft2x13: HIP_TRY(launch_rfft_2x13(fwd, d, p->tabs, batch, p->di, s, off)); break;
    case FftRoute::Rfft2x14: HIP_TRY(launch_rfft_lds15(fwd, d, p->tabs, batch, p->di, s, off)); break;
    case FftRoute::RealRes16:
      if (fwd) HIP_TRY(launch_rfft_res16(d, o, scratch, p->tabs.res16, p->tabs.w2, batch, p->di, s));
      else HIP_TRY(launch_crfft_res16(d, o, scratch, p->tabs.res16, p->tabs.w2, batch, p->di, s));
      break;
    case FftRoute::FourStepSpread:
    case FftRoute::FourStep: HIP_TRY(launch_fft_4step(sh.logn, fwd, scale, d, scratch, p->tabs, batch, p->di, s, o - d)); break;
    case FftRoute::Res16: {
      ResRecord *rec = (ResRecord *)p->res16_rec.p;
      if (rec) p->rec_grid = (int)(batch < p->di.num_cus ? batch : p->di.num_cus);
      HIP_TRY(launch_fft_res16(fwd, scale, d, o, scratch, p->tabs.res16, batch, p->di, s, p->res16_static ? nullptr : p->res16_ctr, rec));
      break;
    }
    case FftRoute::Big: {
      const int e = for_chunks(batch, (long)(p->scratch.bytes / (sizeof(cpx) * (size_t)sh.n)), [&](long b0, long nb) -> int {
        HIP_TRY(launch_fft_big(p->big, fwd, scale, d + b0 * (long)sh.n, o + b0 * (long)sh.n, scratch, (cpx *)p->scratch2.p,
                               (const cpx *)p->bigtabs.p, p->tabs, nb, p->di, s));
        return CLFA_SUCCESS;
      });
      if (e) return e;
      break;
    }
    case FftRoute::BlueLds:   // one launch, one read and one write of the data (fft_aux.inc, k_blue_lds)
      HIP_TRY(launch_blue_lds(sh.blue_m, d, o, (const cpx *)p->blue_w.p, (const cpx *)p->blue_b.p, p->blue_f->tabs.half, sh.n,
                              (scale ? 1.0f / (float)sh.n : 1.0f) / (float)sh.blue_m, batch, p->di, s));
      break;
    case FftRoute::Bluestein:
      if (int e = blue_exec(p, d, o, batch, s)) return e;
      break;
  }
  if (apart && fwd) HIP_TRY(launch_r2c_pack(o, p->tabs.w2, sh.n, batch, s));
  return CLFA_SUCCESS;
}

int clfa_fft_exec_dev(clfa_fft *p, void *data, long batch, void *stream) {
  if (int e = obj_error(p)) return e;
  if (!data || batch < 0) return CLFA_INVALID_VALUE;
  if (batch == 0) return CLFA_SUCCESS;
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;  // NULL is the HIP default stream
  HIP_TRY(p->order.use(s));
  return fft_exec(p, (cpx *)data, 0, batch, s);
}

int clfa_fft_exec_dev_oop(clfa_fft *p, const void *src, void *dst, long batch, void *stream) {
  if (int e = obj_error(p)) return e;
  if (!src || !dst || batch < 0) return CLFA_INVALID_VALUE;
  if (src == dst) return clfa_fft_exec_dev(p, dst, batch, stream);
  if (batch == 0) return CLFA_SUCCESS;
  const size_t bytes = sizeof(cpx) * (size_t)p->sh.n * (size_t)batch;   // real plans: n = size / 2 packed bins = size floats
  const char *a = (const char *)src, *b = (const char *)dst;
  if (spans_overlap(a, bytes, b, bytes)) return CLFA_INVALID_VALUE;  // partly overlapping
  if ((b - a) % (long)sizeof(cpx)) return CLFA_INVALID_VALUE;         // the two buffers a whole number of complex values apart
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  // every kernel reads the source and writes the destination (the kernels take the distance between the two); the source
  // is never written — also not by the routes of several passes, whose first pass already lands in the destination
  return fft_exec(p, (cpx *)const_cast<void *>(src), (long)((b - a) / (long)sizeof(cpx)), batch, s);
}

// ---- measurement aid: what every workgroup of the resident n = 65536 kernel did in the plan's last launch ----
int clfa_fft_balance_record(clfa_fft *p, int on) {
  if (int e = obj_error(p)) return e;
  if (!p->res16_ctr) return CLFA_INVALID_OPERATION;   // no complex n = 65536 plan
  ENTER_DEVICE(p->di.device);
  HIP_TRY(hipDeviceSynchronize());
  p->rec_grid = 0;
  if (!on) {
    p->res16_rec.release();
    return CLFA_SUCCESS;
  }
  return p->res16_rec.ensure(sizeof(ResRecord) * (size_t)p->di.num_cus);
}

int clfa_fft_balance_read(clfa_fft *p, void *records, int max_records, int *count) {
  if (int e = obj_error(p)) return e;
  if (!records || !count || max_records < 0) return CLFA_INVALID_VALUE;
  *count = 0;
  if (!p->res16_rec.p) return CLFA_INVALID_OPERATION;
  ENTER_DEVICE(p->di.device);
  HIP_TRY(hipDeviceSynchronize());   // the launch may be on any stream
  const int n = p->rec_grid < max_records ? p->rec_grid : max_records;
  if (n) HIP_TRY(hipMemcpy(records, p->res16_rec.p, sizeof(ResRecord) * (size_t)n, hipMemcpyDeviceToHost));
  *count = n;
  return CLFA_SUCCESS;
}

// ---- test aid: the counters' lines as they stand, with the guard line on either side ----
int clfa_fft_balance_counters(clfa_fft *p, unsigned *words, int max_words, int *count) {
  if (int e = obj_error(p)) return e;
  if (!words || !count || max_words < 0) return CLFA_INVALID_VALUE;
  *count = 0;
  if (!p->res16_ctr) return CLFA_INVALID_OPERATION;
  ENTER_DEVICE(p->di.device);
  HIP_TRY(hipDeviceSynchronize());   // the launch may be on any stream
  const int all = (int)((kRes16CtrBytes + 2 * kRes16GuardBytes) / sizeof(unsigned));
  const int n = all < max_words ? all : max_words;
  if (n) HIP_TRY(hipMemcpy(words, (const char *)p->res16_ctr - kRes16GuardBytes, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToHost));
  *count = n;
  return CLFA_SUCCESS;
}

int clfa_fft_device_buffers(clfa_fft *p, void **data1, void **data2, void **commands) {
  if (int e = obj_error(p)) return e;
  ENTER_DEVICE(p->di.device);
  const size_t bytes = sizeof(cpx) * (size_t)p->sh.n;
  int e = p->own1.ensure(bytes);
  if (!e) e = p->own2.ensure(bytes);
  if (e) return e;
  if (data1) *data1 = p->own1.p;
  if (data2) *data2 = p->own2.p;
  if (commands) *commands = (void *)p->stream;
  return CLFA_SUCCESS;
}

int clfa_fft_device_tables(clfa_fft *p, void **w, void **b) {
  if (int e = obj_error(p)) return e;
  if (p->sh.blue_m || p->sh.logn < 1 || p->sh.logn > kMaxLog) return CLFA_INVALID_OPERATION;
  ENTER_DEVICE(p->di.device);
  const int n = p->sh.n;
  if (!p->own_tables_ready) {
    std::vector<cpx> tw;
    fill_twiddle(tw, n, n, 1, p->sh.fwd ? -1.f : 1.f);                 // cl_fft.cpp:86-91
    std::vector<int> br((size_t)n);
    int e = clfa_bitrev_table(n, br.data());                        // cl_fft.cpp:96-101
    if (!e) e = p->own_w.ensure(sizeof(cpx) * (size_t)n);
    if (!e) e = p->own_b.ensure(sizeof(int) * (size_t)n);
    if (!e) e = map_hip(hipMemcpy(p->own_w.p, tw.data(), sizeof(cpx) * (size_t)n, hipMemcpyHostToDevice));
    if (!e) e = map_hip(hipMemcpy(p->own_b.p, br.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    if (e) {   // all or nothing: a later call must not hand out a table that was never filled
      (void)hipGetLastError();
      p->own_w.release();
      p->own_b.release();
      return e;
    }
    p->own_tables_ready = true;
  }
  if (w) *w = p->own_w.p;
  if (b) *b = p->own_b.p;
  return CLFA_SUCCESS;
}

int clfa_copy_to_device(void *stream, void *dst, const void *src, size_t bytes, int blocking) {
  if ((!dst || !src) && bytes) return CLFA_INVALID_VALUE;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  if (blocking) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return CLFA_SUCCESS;
}
int clfa_copy_from_device(void *stream, void *dst, const void *src, size_t bytes, int blocking) {
  if ((!dst || !src) && bytes) return CLFA_INVALID_VALUE;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  if (blocking) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return CLFA_SUCCESS;
}
int clfa_stream_synchronize(void *stream) {
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return CLFA_SUCCESS;
}

int clfa_fft_run_buffers(clfa_fft *p) {
  if (int e = obj_error(p)) return e;
  if (!p->own1.p || !p->own2.p) return CLFA_INVALID_MEM_OBJECT;
  if (!p->sh.real) return clfa_fft_exec_dev_oop(p, p->own1.p, p->own2.p, 1, p->stream);
  // a Clrfft's fft() is the complex transform of its N = size / 2 points and nothing else: the reference's conv / iconv
  // are kernels of their own, enqueued by Clrfft::transform (cl_fft.cpp:267-296), not by fft()
  if (!p->own_cplx) {
    const int e = clfa_cfft_create(&p->own_cplx, p->di.device, p->sh.n, p->sh.fwd ? 1 : 0);
    if (e) {
      if (p->own_cplx) clfa_fft_destroy(p->own_cplx);
      p->own_cplx = nullptr;
      return e;
    }
  }
  return clfa_fft_exec_dev_oop(p->own_cplx, p->own1.p, p->own2.p, 1, p->stream);
}

// bytes per call up to which the host entry points go zero-copy: the kernels read the input from,
// and write the result to, mapped pinned host memory (one pass each way), instead of two
// hipMemcpyAsync calls of 10-15 us each around a kernel of a few microseconds
#ifndef CLFA_ZEROCOPY_MAX_KIB
#define CLFA_ZEROCOPY_MAX_KIB 512   // (profiles/host_path_r05.txt: one N = 65536 transform, 512 KiB: 59.5 us this way, 73.5 by copies)
#endif
constexpr size_t kZeroCopyMax = (size_t)CLFA_ZEROCOPY_MAX_KIB << 10;   // (the convolutions': conv_host.hpp)

// ---- pinned arrays for the caller (extension) --------------------------------------------------------------------
// The reference's transform() copies the caller's array to the device and back with two blocking transfers
// (cl_fft.cpp:155-158).  A caller that keeps ONE array for the object's life — the Csound opcodes do: one buffer per
// instance, csound/opcode.cpp — can take that array FROM the plan: page-locked host memory mapped into the device's
// address space.  transform() calls on arrays inside it run on that memory directly (the kernels read and write it over
// PCIe, one pass each way, no staging copy, one synchronisation).
// Why the plan allocates instead of pinning the caller's own array: hipHostRegister on heap arrays was built and measured
// first (round 5) — with arrays registered, unregistered, freed and their addresses reused by arrays of other sizes it
// produced wrong results in 8 of 3000 randomised calls and one GPU memory access fault on a host heap address
// (tools/stress_pinned.py; profiles/host_path_r05.txt) although every array was unregistered before it was freed.
// Memory of hipHostMalloc is the route the staging buffers have used since round 1.
int clfa_fft_host_alloc(clfa_fft *p, size_t bytes, void **ptr) {
  if (!p || !ptr) return CLFA_INVALID_VALUE;
  *ptr = nullptr;
  if (p->err) return p->err;
  if (!bytes) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(p->di.device);
  void *h = nullptr, *d = nullptr;
  hipError_t e = hipHostMalloc(&h, bytes, hipHostMallocMapped);
  if (e == hipSuccess && (e = hipHostGetDevicePointer(&d, h, 0)) != hipSuccess) (void)hipHostFree(h);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return map_hip(e);
  }
  p->pinned.push_back({(char *)h, (char *)d, bytes});
  *ptr = h;
  return CLFA_SUCCESS;
}
int clfa_fft_host_free(clfa_fft *p, void *ptr) {
  if (!p) return CLFA_INVALID_VALUE;
  for (size_t i = 0; i < p->pinned.size(); i++)
    if (p->pinned[i].h == (char *)ptr) {
      ENTER_DEVICE(p->di.device);
      if (p->stream) (void)hipStreamSynchronize(p->stream);
      (void)hipHostFree(ptr);
      p->pinned.erase(p->pinned.begin() + (long)i);
      return CLFA_SUCCESS;
    }
  return CLFA_INVALID_VALUE;
}
// device view of [h, h + bytes) if it lies inside a pinned range, else NULL
static void *pinned_dev(const clfa_fft *p, const void *h, size_t bytes) {
  for (auto &r : p->pinned)
    if ((const char *)h >= r.h && (const char *)h + bytes <= r.h + r.bytes) return r.d + ((const char *)h - r.h);
  return nullptr;
}
// Pinned arrays up to this size run zero-copy when the batch's route touches its source and its destination once each
// (route_one_touch, fft_route.hpp); beyond it, and on the other routes, they are copied by DMA like pageable arrays, only
// faster.
constexpr size_t kPinnedZeroCopyMax = (size_t)8 << 20;

// The blocking host-pointer transforms: src -> dst, which are equal (Clcfft, in place) or the caller's two arrays (Clrfft).
static int fft_host_transform(clfa_fft *p, char *src, char *dst, long batch) {
  ENTER_DEVICE(p->di.device);
  const size_t per = sizeof(cpx) * (size_t)p->sh.n, bytes = per * (size_t)batch;   // real plans: size floats == M complex
  if (batch > 0 && bytes <= kPinnedZeroCopyMax && route_one_touch(fft_route(p->sh, batch), p->sh.real)) {
    // arrays of clfa_fft_host_alloc, both (or the one, in place): the kernels run on them over PCIe
    // (profiles/host_path_r05.txt: N = 65536 42.2 us; with the copy engine bringing the array in first 46.4).  Two arrays
    // that overlap, or lie no whole number of complex values apart, go the ways below like pageable ones.
    char *ds = (char *)pinned_dev(p, src, bytes), *dd = src == dst ? ds : (char *)pinned_dev(p, dst, bytes);
    if (ds && dd && (ds == dd || (!spans_overlap(ds, bytes, dd, bytes) && (dd - ds) % (long)sizeof(cpx) == 0))) {
      const int e = clfa_fft_exec_dev_oop(p, ds, dd, batch, p->stream);
      if (e) return e;
      HIP_TRY(hipStreamSynchronize(p->stream));
      return CLFA_SUCCESS;
    }
  }
  if (batch > 0 && bytes <= kZeroCopyMax) {
    int e = p->zstage.ensure(bytes);
    if (e) return e;
    memcpy(p->zstage.h, src, bytes);
    if ((e = clfa_fft_exec_dev(p, p->zstage.d, batch, p->stream))) return e;
    HIP_TRY(hipStreamSynchronize(p->stream));
    memcpy(dst, p->zstage.h, bytes);
    return CLFA_SUCCESS;
  }
  // staging in chunks of at most 256 MiB, so that huge host batches do not need a device buffer of their full size
  return for_chunks(batch, chunk_items(per, (size_t)256 << 20), [&](long b0, long nb) -> int {
    int e = p->stage.ensure(per * nb);
    if (e) return e;
    HIP_TRY(hipMemcpyAsync(p->stage.p, src + per * b0, per * nb, hipMemcpyHostToDevice, p->stream));   // cl_fft.cpp:155
    if ((e = clfa_fft_exec_dev(p, p->stage.p, nb, p->stream))) return e;                               // cl_fft.cpp:157
    HIP_TRY(hipMemcpyAsync(dst + per * b0, p->stage.p, per * nb, hipMemcpyDeviceToHost, p->stream));   // cl_fft.cpp:158
    HIP_TRY(hipStreamSynchronize(p->stream));
    return CLFA_SUCCESS;
  });
}

int clfa_cfft_transform(clfa_fft *p, float *c, long batch) {
  if (int e = obj_error(p)) return e;
  if (!c || batch < 0 || p->sh.real) return CLFA_INVALID_VALUE;
  return fft_host_transform(p, (char *)c, (char *)c, batch);
}

// forward reads r and writes c; inverse reads c and writes r (cl_fft.cpp:272-294)
int clfa_rfft_transform(clfa_fft *p, float *c, float *r, long batch) {
  if (int e = obj_error(p)) return e;
  if (!c || !r || batch < 0 || !p->sh.real) return CLFA_INVALID_VALUE;
  return fft_host_transform(p, (char *)(p->sh.fwd ? r : c), (char *)(p->sh.fwd ? c : r), batch);
}

int clfa_reorder_dev(int device, void *out, const void *in, int n, long batch, void *stream) {
  if (!out || !in || out == in || !is_pow2(n) || n < 2 || batch < 0) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(device);
  HIP_TRY(launch_reorder((cpx *)out, (const cpx *)in, ilog2(n), batch, (hipStream_t)stream));
  return CLFA_SUCCESS;
}

}  // extern "C"
