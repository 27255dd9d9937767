// fs_abi.hip - host side of libflowsim_hip.so: the C ABI declared in include/flowsim_abi.h.
//
// Holds the device buffers of a batch (SoA, reach-major state [B][N]; per-level tables [level][B]) as fs::DeviceBuffer /
// fs::PinnedBuffer members (fs_buffer.hpp: freed with the handle), converts caller float64 host arrays to the batch dtype on
// upload, asks fs::pick (fs_dispatch.hpp) for the kernel instantiation and launches the fused step kernel on the handle's HIP
// stream.  What needs no device - packing polylines and stage tables, extending geometry tables, validating boundary arguments
// (fs_host_pack.hpp), the checks and result layouts of post-processing (fs_host_post.hpp) - the CPU tests build on its own; the batch's
// arithmetic type becomes a C++ type in one place (with_real).  No CPU compute path: without a device every entry point that needs one says so.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "fs_balance.hpp"
#include "fs_buffer.hpp"
#include "fs_entries.hpp"
#include "fs_envelope.hpp"
#include "fs_forcing.hpp"
#include "fs_gauge.hpp"
#include "fs_assim.hpp"
#include "fs_host_pack.hpp"
#include "fs_host_post.hpp"
#include "fs_init_state.hpp"
#include "fs_member_geo.hpp"
#include "fs_reduce.hpp"

// ROCTx ranges around the phases a system trace should show (rocprofv3 --marker-trace): uploads, downloads, the step launch,
// the post-processing launch.  Without a tool attached a push / pop is a few nanoseconds.
#include <rocprofiler-sdk-roctx/roctx.h>
namespace {
struct TraceRange {
  explicit TraceRange(const char *name) { roctxRangePushA(name); }
  ~TraceRange() { roctxRangePop(); }
};
}  // namespace

#ifndef FS_MINIMAL
// the library: the kernels are instantiated in the fs_part_*.hip translation units (an FS_MINIMAL build instantiates its few where the
// table below takes their address)
FS_ACTIVE_LIST(FS_DECLARE)
#else
// an experiment build is this translation unit alone, with a few step kernels: it has no initial-condition kernels (fs_part_init.hip)
// no post-processing kernels (fs_part_reduce.hip, fs_part_envelope.hip, fs_part_balance.hip, fs_part_gauges.hip, fs_part_assim.hip), no forcing kernels (fs_part_forcing.hip) and no geometry kernels
// (fs_part_geometry.hip), and fs_batch_init_state, fs_batch_summarize, fs_batch_set_bc_sampled ... say so
namespace fs {
bool launch_envelope(const EnvelopeArgs<double> &, int, hipStream_t) { return false; }
bool launch_envelope(const EnvelopeArgs<float> &, int, hipStream_t) { return false; }
bool launch_transpose_rows(const TransposeRows &, int, double *, int, int, hipStream_t) { return false; }
bool launch_profile_bands(const ProfileBandArgs &, hipStream_t) { return false; }
bool launch_reach_integrals(const IntegralArgs<double> &, hipStream_t) { return false; }
bool launch_reach_integrals(const IntegralArgs<float> &, hipStream_t) { return false; }
bool launch_balance(const ReduceArgs<double> &, const BalanceArgs &, hipStream_t) { return false; }
bool launch_balance(const ReduceArgs<float> &, const BalanceArgs &, hipStream_t) { return false; }
bool launch_clear_integrals(double *, size_t, int32_t *, size_t, hipStream_t) { return false; }
bool launch_gauge_gather(const GaugeArgs<double> &, bool, hipStream_t) { return false; }
bool launch_gauge_gather(const GaugeArgs<float> &, bool, hipStream_t) { return false; }
bool launch_gauge_score(const ReduceArgs<double> &, const ScoreArgs &, hipStream_t) { return false; }
bool launch_gauge_members(const int32_t *, const int32_t *, const int32_t *, const double *, int, int, int, int, int, int32_t *, hipStream_t) { return false; }
bool launch_assimilate(const AssimArgs<double> &, hipStream_t) { return false; }
bool launch_assimilate(const AssimArgs<float> &, hipStream_t) { return false; }
bool launch_member_sections(const MemberGeoArgs &, hipStream_t) { return false; }
bool launch_member_tables(const MemberGeoArgs &, hipStream_t) { return false; }
bool launch_sample_target(const SampleArgs<double> &, hipStream_t) { return false; }
bool launch_sample_target(const SampleArgs<float> &, hipStream_t) { return false; }
bool launch_route_pool(const PoolArgs<double> &, hipStream_t) { return false; }
bool launch_route_pool(const PoolArgs<float> &, hipStream_t) { return false; }
bool launch_init_state(int, const InitArgs<double> &, hipStream_t) { return false; }
bool launch_init_state(int, const InitArgs<float> &, hipStream_t) { return false; }
bool launch_summarize(const ReduceArgs<double> &, double *, hipStream_t) { return false; }
bool launch_summarize(const ReduceArgs<float> &, double *, hipStream_t) { return false; }
bool launch_lookup(const ReduceArgs<double> &, const LookupArgs &, hipStream_t) { return false; }
bool launch_lookup(const ReduceArgs<float> &, const LookupArgs &, hipStream_t) { return false; }
bool launch_bands(const ReduceArgs<double> &, const BandArgs &, hipStream_t) { return false; }
bool launch_bands(const ReduceArgs<float> &, const BandArgs &, hipStream_t) { return false; }
}  // namespace fs
#endif

namespace {

thread_local std::string g_err;

int fail(const std::string &m) { g_err = m; return -1; }

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));   \
  } while (0)

// Every entry point that allocates, copies, launches or frees runs with the batch's device current and puts the
// caller's device back on the way out (two batches on different ordinals in one process, calls from another thread).
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define FS_ON_DEVICE(b)                                                                     \
  DeviceGuard guard_((b)->d.device);                                                        \
  if (!guard_.ok) return fail("hipSetDevice(" + std::to_string((b)->d.device) + ") failed")

// the dispatch table: what each instantiation was compiled for (fs::KernelKey, fs_dispatch.hpp), its launcher and its kernel.  Which
// entry a batch gets: fs::pick
struct Entry { fs::KernelKey key; FsLaunchFn fn; const void *kp; };
const Entry kEntries[] = {FS_ACTIVE_LIST(FS_TABLE_ROW)};
constexpr int kNumEntries = (int)(sizeof(kEntries) / sizeof(kEntries[0]));

}  // namespace

// ---------------------------------------------------------------------------------------------
// Host <-> device staging.  Large transfers go through a ring of pinned chunks (hipHostMalloc): while the DMA engine moves
// chunk i, a few host threads copy (and, for fp32 batches, convert) chunk i + 1 between the caller's pageable buffer and
// the next pinned chunk - the host copy, the page faults of a freshly allocated destination and the PCIe transfer overlap
// instead of adding up.  (A pageable hipMemcpy device -> host measured 22.9 GB/s on this box, profiles/round2/pcie.json.)
// ---------------------------------------------------------------------------------------------
namespace {

class CopyPool {                       // a handful of persistent host threads: parallel_for over slices of a chunk
 public:
  static CopyPool &get() { static CopyPool p; return p; }
  int size() const { return (int)workers_.size() + 1; }
  void run(size_t n, const std::function<void(size_t, size_t)> &fn) {        // fn(begin, end) over [0, n)
    const int parts = size();
    if (n < (size_t)1 << 16 || parts == 1) { fn(0, n); return; }
    std::lock_guard<std::mutex> one_at_a_time(run_m_);        // handles on different host threads share the pool
    {
      std::lock_guard<std::mutex> lk(m_);
      fn_ = &fn; n_ = n; parts_ = parts; pending_ = parts - 1; ++epoch_;
    }
    cv_.notify_all();
    slice(parts - 1);
    std::unique_lock<std::mutex> lk(m_);
    done_.wait(lk, [&] { return pending_ == 0; });
  }

 private:
  CopyPool() {
    const char *env = std::getenv("FS_COPY_THREADS");
    int want = env ? std::atoi(env) : (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency() / 2));
    want = std::max(1, std::min(want, 32));
    for (int i = 0; i + 1 < want; ++i) workers_.emplace_back([this, i] { loop(i); });
  }
  ~CopyPool() {
    { std::lock_guard<std::mutex> lk(m_); stop_ = true; ++epoch_; }
    cv_.notify_all();
    for (auto &t : workers_) t.join();
  }
  void slice(int part) {
    const size_t per = (n_ + parts_ - 1) / parts_, a = std::min(n_, per * part), b = std::min(n_, a + per);
    if (a < b) (*fn_)(a, b);
  }
  void loop(int id) {
    unsigned long seen = 0;
    for (;;) {
      std::unique_lock<std::mutex> lk(m_);
      cv_.wait(lk, [&] { return epoch_ != seen; });
      seen = epoch_;
      if (stop_) return;
      lk.unlock();
      slice(id);
      lk.lock();
      if (--pending_ == 0) done_.notify_one();
    }
  }
  std::vector<std::thread> workers_;
  std::mutex m_, run_m_;
  std::condition_variable cv_, done_;
  const std::function<void(size_t, size_t)> *fn_ = nullptr;
  size_t n_ = 0;
  int parts_ = 1, pending_ = 0;
  unsigned long epoch_ = 0;
  bool stop_ = false;
};

constexpr size_t kStageChunk = (size_t)32 << 20;      // bytes per pinned chunk
constexpr int kStageSlots = 3;
constexpr size_t kStageMin = (size_t)8 << 20;         // smaller transfers: one plain copy

struct Staging {
  fs::PinnedBuffer buf[kStageSlots];
  hipEvent_t ev[kStageSlots] = {nullptr, nullptr, nullptr};
  bool ready = false;
  int init() {
    if (ready) return 0;
    for (int i = 0; i < kStageSlots; ++i) {
      if (buf[i].ensure(kStageChunk) != hipSuccess) return -1;
      if (!ev[i] && hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return -1;
    }
    ready = true;
    return 0;
  }
  ~Staging() {
    for (int i = 0; i < kStageSlots; ++i) {
      buf[i].reset();
      if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
  }
};

// the stream and the two timing events of a batch: a base of fs_batch, so that they outlive its buffers
struct Timeline {
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~Timeline() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

}  // namespace

struct fs_batch : Timeline {
  fs_batch_desc d;
  size_t esz;                 // sizeof(real)
  bool timed = false;
  bool iterating = false;     // a level opened by fs_batch_iterate has not been closed yet
  int launches = 0;
  int level = 0;
  int restart_level = 0;      // > 0: the batch was re-seeded at this level (fs_batch_restart); history rows 1 .. restart_level-1 are empty
  const Entry *kern = nullptr;
  // scheme
  double theta = 0.6, dt = 0, dx = 0, tol = 1e-4;
  int max_iter = 100;
  bool have_scheme = false, have_geo = false, have_state = false, have_bc[2] = {false, false};
  // device buffers (an empty one reads as nullptr: the kernels take that as "not given")
  fs::DeviceBuffer hk, Qk, hg, Qg;
  fs::DeviceBuffer geo_uniform, geo_table, n_override;
  fs::DeviceBuffer poly_x, poly_z, poly_lim, poly_n;     // poly_n: int32
  fs::DeviceBuffer poly_tz;             // stage tables of the polylines (fs_poly.hpp)
  int poly_K = 0;
  int poly_P = 0;                       // max_pts of the polylines on the device
  fs::DeviceBuffer member_in[9];        // double / int32: fs_batch_set_geometry_irregular_members' shared channel (x, z, limits, n_pts, table) and transforms (dz_left, dz_main, dz_right, n_scale)
  size_t geo_reach_stride = 0, poly_reach_stride = 0;     // per-reach geometry (elements between the tables of two reaches), 0: shared
  fs::DeviceBuffer reach_nodes;         // int32 [B] per-reach node counts (heterogeneous batch) or empty
  std::vector<int32_t> reach_nodes_host;      // its host copy (empty: every reach has n_nodes): where a reach's last node is
  bool any_storage[2] = {false, false}; // some reach's boundary on this side is a storage kind (per-reach kinds: OR over the reaches)
  fs::DeviceBuffer reach_scheme;        // [5][B] per-reach theta, dt, dx, tolerance, max_iter or empty
  std::vector<double> rs_host[5];       // what the caller set per reach (empty: the batch-wide value of fs_batch_set_scheme)
  fs::DeviceBuffer reach_kinds;         // int32 [2][B] per-reach boundary kinds or empty
  bool kinds_per_reach[2] = {false, false};
  bool some_host_rows[2] = {false, false};      // per-reach kinds with FS_BC_HOST_ROW among them: fs_batch_set_host_rows writes those reaches' rows only
  fs::DeviceBuffer rows_stage;          // [3][B] what the caller handed to fs_batch_set_host_rows, before the masked merge into the parameters
  fs::DeviceBuffer bc_params[2], bc_target[2];
  int bc_kind[2] = {0, 0}, bc_stride[2] = {0, 0};
  fs::DeviceBuffer Yprev, stage_hist, trace, hydro, hist_h, hist_Q;
  fs::DeviceBuffer iters, status;       // int32
  fs::DeviceBuffer it_done;             // int32 [B] Newton iterations spent on the open level (fs_batch_iterate)
  fs::DeviceBuffer ends_dev;            // double [4][B] scratch of fs_batch_get_boundary_iterate (allocated on first use)
  fs::PinnedBuffer ends_pin;            // its pinned host mirror
  fs::DeviceBuffer open_dev;            // int32: fs_batch_iterate's count of the reaches still iterating
  fs::PinnedBuffer open_pin;
  fs::DeviceBuffer derived[8];          // device results of the last derive call, kept and reused (grown, never shrunk)
  fs::DeviceBuffer ic_in[4];            // fs_batch_init_state's inputs in the batch's type: flow, depth_us, depth_ds [B], bed_slope [N] or [B][N]
  fs::DeviceBuffer ic_info;             // int32 [2][B]: what fs_batch_init_state reports per reach (allocated on first use)
  fs::DeviceBuffer red_in[3];           // double: what the caller handed to the last fs_batch_lookup / fs_batch_bands (offsets, abscissae or levels, targets)
  fs::DeviceBuffer red_out[3];          // results of the last fs_batch_summarize / lookup / bands, kept and reused (grown, never shrunk)
  fs::DeviceBuffer env_out;             // double [env_rows][B][N]: the last fs_batch_envelope - its (quantity, statistic) rows, then its crossings (grown, never shrunk)
  fs::DeviceBuffer env_levels;          // int32 [B]: the rows of each reach that entered it
  fs::DeviceBuffer env_thr;             // the threshold it was handed, in the batch's type: [N] or [B][N]
  fs::DeviceBuffer env_t;               // double [2][N][B]: fs_batch_profile_bands' transposed row and crossing counts
  fs::DeviceBuffer integ;               // double [max_levels][FS_INT_NROWS][B]: reach integrals and balance residuals, NaN where never evaluated (allocated on first use)
  fs::DeviceBuffer integ_mark;          // int32 [max_levels][B]: 1 where a row of integ holds integrals
  fs::DeviceBuffer integ_thr;           // the threshold fs_batch_reach_integrals was handed, in the batch's type: [N] or [B][N]
  fs::DeviceBuffer bal_scheme;          // double [3][B]: theta, dt, dx of each reach as the caller gave them in fp64 (rs_host, else the batch's)
  bool bal_scheme_stale = true;         // the scheme changed since bal_scheme was uploaded
  fs::DeviceBuffer gauge;               // double [n_gauges][max_levels][FS_GAUGE_NROWS][B]: the gauge rows, NaN where never evaluated (fs_batch_set_gauges)
  fs::DeviceBuffer gauge_mark;          // int32 [max_levels][B]: bit g set where gauge g's row holds values
  fs::DeviceBuffer gauge_node, gauge_weight;      // int32 / double [n_gauges], or [B][n_gauges] with gauge_per_reach
  fs::DeviceBuffer gauge_members;       // int32 [B]: fs_batch_gauge_bands' status of each member at the gauge it was asked for
  int n_gauges = 0;
  bool gauge_per_reach = false;
  fs::DeviceBuffer assim_part;          // double [chunks][2][n_obs + 2][N]: the partial sums of the last fs_batch_assimilate (grown, never shrunk)
  fs::DeviceBuffer assim_out;           // double: its prior [4][N], then its cross covariances [2][n_obs][N]
  fs::DeviceBuffer assim_cols;          // double: its S, then its Z, both [B][bucket]
  fs::DeviceBuffer assim_taper;         // double [n_obs][N]: the taper it was handed
  fs::DeviceBuffer assim_flags;         // int32: the active flags [B], then the clamped counts [B]
  std::vector<char> gauge_levels;       // [max_levels]: 1 where fs_batch_gauges has evaluated the level since the last reset
  int env_quantities = 0;               // FS_ENV_* mask of the envelope the handle holds (0: none)
  bool env_crossings = false;           // ... and whether it has crossing rows
  fs::DeviceBuffer frc_in[2][6];        // double / int32: what fs_batch_set_bc_sampled was handed per side (times, values, table_of, scale, offset, shift)
  fs::DeviceBuffer frc_dt;              // double [B]: the per-reach time steps as the caller gave them (the forcing kernels compute in fp64), or empty
  fs::DeviceBuffer pool_in[5];          // double: fs_batch_route_pool's curve stages, curve volumes, weirs, initial stages, weir multipliers
  fs::DeviceBuffer pool_stage;          // double [max_levels][B]: the pool stages of the last fs_batch_route_pool
  fs::DeviceBuffer pool_info;           // int32 [2][B]: what it reports per member
  fs::DeviceBuffer dbg;
  Staging stage;                        // pinned chunks for large host <-> device transfers
  fs::DeviceBuffer kc_scratch;          // long reaches: level constants [B][4][passes * 64 W M]
  fs::DeviceBuffer hk_entry, Qk_entry;  // long reaches of uniform sections: the state a launch of several levels began with (restore_failed_state)
  fs::DeviceBuffer Yprev_entry;         // storage boundaries: the reservoir stages a launch of several levels began with (restore_failed_stage)
  int passes = 0;
  fs::DeviceBuffer team_mail;           // reaches stepped by teams of workgroups: mailboxes [B][2][G W + 1][kTeamWords]
  fs::DeviceBuffer team_sync;           // uint64 [1]: the ticket counter, zeroed before every launch
  int team_size = 0;
  uint32_t team_epoch = 0;              // team launches made on this handle (the high half of the tagged mailbox's tags)
};

namespace {

// the batch's arithmetic type as a C++ type: f(double()) or f(float())
template <typename F> auto with_real(const fs_batch *b, F &&f) { return b->d.dtype == FS_F64 ? f(double()) : f(float()); }

// one thread per item (reach, or node of the batch), 256 per block
dim3 grid_256(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

// n doubles of the caller's into device memory that holds at least n elements of the batch's type
int upload_to(fs_batch *b, void *dst, const double *src, size_t n) {
  TraceRange range_("flowsim:upload");
  const bool f64 = b->esz == sizeof(double);
  if (f64 || n * b->esz < kStageMin || b->stage.init() != 0) {
    // fp64: the runtime's own pageable path (it pins and pipelines; ~55 GB/s here); small fp32 arrays: convert, then one copy
    if (f64) {
      HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, b->stream));
      HIP_TRY(hipStreamSynchronize(b->stream));
    } else {
      std::vector<float> tmp(n);
      for (size_t i = 0; i < n; ++i) tmp[i] = (float)src[i];
      HIP_TRY(hipMemcpyAsync(dst, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice, b->stream));
      HIP_TRY(hipStreamSynchronize(b->stream));
    }
    return 0;
  }
  // fp32, large: convert chunk i + 1 into a pinned slot (host threads) while chunk i is on the bus
  const size_t per = kStageChunk / sizeof(float);
  int slot = 0;
  for (size_t off = 0; off < n; off += per, slot = (slot + 1) % kStageSlots) {
    const size_t cnt = std::min(per, n - off);
    HIP_TRY(hipEventSynchronize(b->stage.ev[slot]));              // the DMA that last read this slot is through
    float *pin = b->stage.buf[slot].get<float>();
    const double *sp = src + off;
    CopyPool::get().run(cnt, [&](size_t lo, size_t hi) { for (size_t i = lo; i < hi; ++i) pin[i] = (float)sp[i]; });
    HIP_TRY(hipMemcpyAsync((char *)dst + off * sizeof(float), pin, cnt * sizeof(float), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipEventRecord(b->stage.ev[slot], b->stream));
  }
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// ... into a buffer of exactly that size
int upload(fs_batch *b, fs::DeviceBuffer &dst, const double *src, size_t n) {
  HIP_TRY(dst.ensure(n * b->esz));
  return upload_to(b, dst.get(), src, n);
}

int download(fs_batch *b, double *dst, const fs::DeviceBuffer &src, size_t off_elems, size_t n) {
  TraceRange range_("flowsim:download");
  HIP_TRY(hipStreamSynchronize(b->stream));
  const bool f64 = b->esz == sizeof(double);
  const char *dev = src.get<const char>() + off_elems * b->esz;
  if (n * b->esz < kStageMin || b->stage.init() != 0) {
    if (f64) {
      HIP_TRY(hipMemcpy(dst, dev, n * 8, hipMemcpyDeviceToHost));
    } else {
      std::vector<float> tmp(n);
      HIP_TRY(hipMemcpy(tmp.data(), dev, n * 4, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n; ++i) dst[i] = tmp[i];
    }
    return 0;
  }
  // chunk i + 1 comes over the bus into a pinned slot while host threads copy (fp32: widen) chunk i into the caller's buffer
  const size_t per = kStageChunk / b->esz, chunks = (n + per - 1) / per;
  auto issue = [&](size_t c) -> hipError_t {
    const int slot = (int)(c % kStageSlots);
    const size_t off = c * per, cnt = std::min(per, n - off);
    hipError_t e = hipMemcpyAsync(b->stage.buf[slot].get(), dev + off * b->esz, cnt * b->esz, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipEventRecord(b->stage.ev[slot], b->stream);
    return e;
  };
  for (size_t c = 0; c < std::min<size_t>(chunks, kStageSlots - 1); ++c) HIP_TRY(issue(c));
  for (size_t c = 0; c < chunks; ++c) {
    const int slot = (int)(c % kStageSlots);
    const size_t off = c * per, cnt = std::min(per, n - off);
    if (c + kStageSlots - 1 < chunks) HIP_TRY(issue(c + kStageSlots - 1));   // its slot was drained in the iteration before
    HIP_TRY(hipEventSynchronize(b->stage.ev[slot]));
    double *dp = dst + off;
    if (f64) {
      const double *pin = b->stage.buf[slot].get<const double>();
      CopyPool::get().run(cnt, [&](size_t lo, size_t hi) { std::memcpy(dp + lo, pin + lo, (hi - lo) * sizeof(double)); });
    } else {
      const float *pin = b->stage.buf[slot].get<const float>();
      CopyPool::get().run(cnt, [&](size_t lo, size_t hi) { for (size_t i = lo; i < hi; ++i) dp[i] = pin[i]; });
    }
  }
  return 0;
}

// the Newton vector at the two ends of every reach, as doubles: out[4][B] = h_0, Q_0, h_last, Q_last (fs_batch_get_boundary_iterate)
template <typename R>
__global__ void gather_boundary_iterate(const R *hg, const R *Qg, const int32_t *reach_nodes, double *out, size_t B, size_t N) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B) return;
  const size_t last = (reach_nodes ? (size_t)reach_nodes[r] : N) - 1;
  out[r] = (double)hg[r * N]; out[B + r] = (double)Qg[r * N];
  out[2 * B + r] = (double)hg[r * N + last]; out[3 * B + r] = (double)Qg[r * N + last];
}

// the downstream half of the level-0 hydrograph row from the state on the device: node reach_nodes[r] - 1 of every reach
// (fs_batch_set_reach_nodes after fs_batch_set_state: the row was filled from column N - 1)
template <typename R>
__global__ void refresh_level0_downstream(const R *hk, const R *Qk, const int32_t *reach_nodes, R *hydro, size_t B, size_t N) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B) return;
  const size_t last = (reach_nodes ? (size_t)reach_nodes[r] : N) - 1;
  hydro[2 * B + r] = hk[r * N + last]; hydro[3 * B + r] = Qk[r * N + last];
}

// ... and the upstream half, from node 0 (fs_batch_init_state: the state was computed on the device)
template <typename R>
__global__ void refresh_level0_upstream(const R *hk, const R *Qk, R *hydro, size_t B, size_t N) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B) return;
  hydro[r] = hk[r * N]; hydro[B + r] = Qk[r * N];
}

// The multi-pass kernel of the uniform section modes reads the accepted state of level k from hk / Qk while it iterates on level
// k + 1 (fs_long.hpp: its level constants are recomputed, not stored), so it writes every accepted level there - also those a reach
// completes before it fails later in the same launch.  fs_batch_get_state promises the state at the end of the previous call for a
// failed reach (include/flowsim_abi.h): the rows of such a reach go back to what the launch began with.
template <typename R>
__global__ void restore_failed_state(const int32_t *status, const R *hk0, const R *Qk0, R *hk, R *Qk, size_t B, size_t N) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * N) return;
  const int32_t st = status[i / N];
  if (st != FS_OK && st != FS_ILL_CONDITIONED) { hk[i] = hk0[i]; Qk[i] = Qk0[i]; }
}

// The same promise for the reservoir stage (fs_batch_get_storage_stage): every step kernel keeps the stage of the last level it
// accepted and writes it back when it ends, also for a reach that failed on a later level of the same launch.
template <typename R>
__global__ void restore_failed_stage(const int32_t *status, const R *Y0, R *Y, size_t B) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B) return;
  const int32_t st = status[r];
  if (st != FS_OK && st != FS_ILL_CONDITIONED) Y[r] = Y0[r];
}

// reaches whose open level still iterates (fs_batch_iterate): not yet accepted and not failed
__global__ void count_open_reaches(const int32_t *done, const int32_t *status, int32_t *out, size_t B) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool open = r < B && done[r] >= 0 && (status[r] == FS_OK || status[r] == FS_ILL_CONDITIONED);   // (a warning, not a failure)
  const unsigned long long m = __ballot(open);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(out, (int32_t)__popcll(m));
}

// fs_batch_set_host_rows on a side with per-reach kinds: the rows of the host-evaluated reaches go into parameter rows 0..2, the
// parameters of the reaches whose kind the device evaluates stay what fs_batch_set_bc_per_reach stored
template <typename R>
__global__ void merge_host_rows(R *params, const R *rows, const int32_t *kinds, size_t B) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B || kinds[r] != FS_BC_HOST_ROW) return;
  for (int i = 0; i < 3; ++i) params[(size_t)i * B + r] = rows[(size_t)i * B + r];
}

// level 0 of every array from one (h, Q) pair per reach
template <typename R>
__global__ void broadcast_state(const R *h, const R *Q, R *hk, R *Qk, R *hg, R *Qg, R *hist_h, R *hist_Q, R *hydro,
                                size_t B, size_t N) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * N) return;
  const size_t r = i / N, node = i - r * N;
  const R hv = h[r], Qv = Q[r];
  hk[i] = hv; Qk[i] = Qv; hg[i] = hv; Qg[i] = Qv;
  if (hist_h) { hist_h[i] = hv; hist_Q[i] = Qv; }
  if (node == 0) { hydro[0 * B + r] = hv; hydro[1 * B + r] = Qv; hydro[2 * B + r] = hv; hydro[3 * B + r] = Qv; }
}

template <typename R> void fill_args(const fs_batch *b, int n_steps, fs::KernelArgs<R> &a) {
  a.B = b->d.n_reaches; a.N = b->d.n_nodes; a.n_steps = n_steps; a.level0 = b->level; a.max_iter = b->max_iter;
  a.theta = (R)b->theta; a.dt = (R)b->dt; a.dx = (R)b->dx; a.tol = (R)b->tol;
  a.hk = b->hk.get<R>(); a.Qk = b->Qk.get<R>(); a.hg = b->hg.get<R>(); a.Qg = b->Qg.get<R>();
  a.geo_uniform = b->geo_uniform.get<R>(); a.geo_table = b->geo_table.get<R>();
  a.n_override = b->n_override.get<R>();
  a.poly_x = b->poly_x.get<R>(); a.poly_z = b->poly_z.get<R>(); a.poly_lim = b->poly_lim.get<R>(); a.poly_n = b->poly_n.get<int32_t>();
  a.poly_tz = b->poly_tz.get<R>(); a.poly_K = b->poly_K;
  a.geo_reach_stride = (int64_t)b->geo_reach_stride; a.poly_reach_stride = (int64_t)b->poly_reach_stride;
  a.reach_nodes = b->reach_nodes.get<int32_t>(); a.reach_scheme = b->reach_scheme.get<R>();
  a.reach_kinds = (b->kinds_per_reach[0] || b->kinds_per_reach[1]) ? b->reach_kinds.get<int32_t>() : nullptr;
  fs::BCDesc<R> *bc[2] = {&a.us, &a.ds};
  for (int s = 0; s < 2; ++s) {
    bc[s]->kind = b->bc_kind[s]; bc[s]->stride = b->bc_stride[s];
    bc[s]->params = b->bc_params[s].get<R>(); bc[s]->target = b->bc_target[s].get<R>(); bc[s]->tgt = R(0);
  }
  a.Yprev = b->Yprev.get<R>(); a.stage_hist = b->stage_hist.get<R>(); a.trace = b->trace.get<R>(); a.hydro = b->hydro.get<R>();
  a.iters = b->iters.get<int32_t>(); a.status = b->status.get<int32_t>();
  a.hist_h = b->hist_h.get<R>(); a.hist_Q = b->hist_Q.get<R>();
  a.dbg = b->dbg.get<unsigned long long>();
  a.kc_scratch = b->kc_scratch.get<R>(); a.passes = b->passes;
  a.team_size = b->team_size; a.team_mail = b->team_mail.get<R>(); a.team_sync = b->team_sync.get<unsigned long long>(); a.team_epoch = b->team_epoch;
  a.iter_budget = 0; a.it_done = b->it_done.get<int32_t>();
}

// picks the instantiation for the batch as it is now (the boundary kinds are known) and launches it on the handle's stream
int launch_steps(fs_batch *b, int n_steps, int iter_budget) {
  TraceRange range_(iter_budget > 0 ? "flowsim:iterate" : "flowsim:step");
  std::string why;
  const int hetero = (b->reach_nodes ? 1 : 0) | ((b->reach_scheme || b->kinds_per_reach[0] || b->kinds_per_reach[1]) ? 2 : 0);
  fs::Query q;
  q.dtype = b->d.dtype; q.sec = b->d.section_mode; q.N = b->d.n_nodes; q.usk = b->bc_kind[0]; q.dsk = b->bc_kind[1];
  q.need_diag = (b->d.flags & (FS_FLAG_HISTORY | FS_FLAG_TRACE | FS_FLAG_MONITOR)) != 0; q.need_any = iter_budget > 0; q.hetero = hetero;
  const int chosen = fs::pick(kEntries, kNumEntries, q, fs::overrides_from_environment(), &why);
  const Entry *k = chosen < 0 ? nullptr : &kEntries[chosen];
  if (!k && why.rfind("FS_KERNEL_INDEX", 0) == 0) return fail("fs_batch_step: " + why);
  if (!k && (b->bc_kind[0] == FS_BC_STORAGE_CURVE || b->bc_kind[1] == FS_BC_STORAGE_CURVE))
    return fail("fs_batch_step: FS_BC_STORAGE_CURVE needs section mode FS_SEC_TABLE or FS_SEC_IRREGULAR");
  if (!k) return fail("fs_batch_step: no kernel instantiation for this boundary kind at this size");
  b->kern = k;
  const size_t B = b->d.n_reaches, N = b->d.n_nodes;
  const fs::LaunchPlan plan = fs::plan_launch(k->key, b->d.section_mode, B, N, n_steps, b->any_storage[FS_DOWNSTREAM]);
  b->passes = plan.passes; b->team_size = plan.team_size;
  HIP_TRY(b->kc_scratch.reserve(plan.kc_scratch_elems * b->esz));
  if (plan.team_size) {    // the mailboxes (zeroed once - a tag is never 0, launches count from 1) and the ticket counter (zero at every launch)
    bool grew = false;
    HIP_TRY(b->team_mail.reserve(plan.team_mail_bytes, &grew));
    if (grew) HIP_TRY(hipMemsetAsync(b->team_mail.get(), 0, plan.team_mail_bytes, b->stream));
    ++b->team_epoch;
    HIP_TRY(b->team_sync.ensure(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(b->team_sync.get(), 0, sizeof(unsigned long long), b->stream));
  }
  if (plan.keep_entry) {
    const size_t state_bytes = B * N * b->esz;
    HIP_TRY(b->hk_entry.reserve(state_bytes));
    HIP_TRY(b->Qk_entry.reserve(state_bytes));
    HIP_TRY(hipMemcpyAsync(b->hk_entry.get(), b->hk.get(), state_bytes, hipMemcpyDeviceToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->Qk_entry.get(), b->Qk.get(), state_bytes, hipMemcpyDeviceToDevice, b->stream));
  }
  if (plan.keep_stage) {
    HIP_TRY(b->Yprev_entry.reserve(B * b->esz));
    HIP_TRY(hipMemcpyAsync(b->Yprev_entry.get(), b->Yprev.get(), B * b->esz, hipMemcpyDeviceToDevice, b->stream));
  }
  HIP_TRY(hipEventRecord(b->ev0, b->stream));
  with_real(b, [&](auto real) {
    using R = decltype(real);
    fs::KernelArgs<R> a; fill_args(b, n_steps, a);
    a.iter_budget = iter_budget;
    b->kern->fn(&a, b->d.n_reaches, b->stream);
    if (plan.keep_entry)
      hipLaunchKernelGGL((restore_failed_state<R>), grid_256(B * N), dim3(256), 0, b->stream, b->status.get<const int32_t>(),
                         b->hk_entry.get<const R>(), b->Qk_entry.get<const R>(), b->hk.get<R>(), b->Qk.get<R>(), B, N);
    if (plan.keep_stage)
      hipLaunchKernelGGL((restore_failed_stage<R>), grid_256(B), dim3(256), 0, b->stream, b->status.get<const int32_t>(),
                         b->Yprev_entry.get<const R>(), b->Yprev.get<R>(), B);
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(b->ev1, b->stream));
  b->timed = true; b->launches = 1;
  return 0;
}

// ---- steps that several entry points share ----

int check_side(const char *entry, int32_t side) {
  if (side != FS_UPSTREAM && side != FS_DOWNSTREAM) return fail(std::string(entry) + ": side must be FS_UPSTREAM or FS_DOWNSTREAM");
  return 0;
}

int check_levels(const fs_batch *b, const char *entry, int32_t first, int32_t n) {
  if (first < 0 || n < 1 || first + n > b->d.max_levels) return fail(std::string(entry) + ": level range out of bounds");
  return 0;
}

int check_ready(const fs_batch *b, const char *entry) {
  if (!b->have_scheme || !b->have_geo || !b->have_state || !b->have_bc[0] || !b->have_bc[1])
    return fail(std::string(entry) + ": scheme, geometry, both boundaries and the initial state must be set first");
  return 0;
}

// the per-reach Manning n of the main channel: the caller's, or none
int set_n_override(fs_batch *b, const double *n_main_override) {
  if (n_main_override) return upload(b, b->n_override, n_main_override, b->d.n_reaches);
  b->n_override.reset();
  return 0;
}

// a side's parameters and target hydrographs replaced by the caller's (params == nullptr: n_params rows of zeros; n_params == 0: none)
int replace_bc_buffers(fs_batch *b, int side, const double *params, size_t n_params, const double *target) {
  b->bc_params[side].reset();
  b->bc_target[side].reset();
  if (params) {
    if (n_params > 0 && upload(b, b->bc_params[side], params, n_params)) return -1;
  } else if (n_params > 0) {
    HIP_TRY(b->bc_params[side].ensure(n_params * b->esz));
    HIP_TRY(hipMemsetAsync(b->bc_params[side].get(), 0, n_params * b->esz, b->stream));
  }
  if (target && upload(b, b->bc_target[side], target, (size_t)b->d.max_levels * b->d.n_reaches)) return -1;
  return 0;
}

// n int32 of the caller's into device memory that holds at least n
int upload_i32(int32_t *dst, const int32_t *src, size_t n) {
  HIP_TRY(hipMemcpy(dst, src, n * sizeof(int32_t), hipMemcpyHostToDevice));
  return 0;
}

// one kind into every slot of a side of reach_kinds
int fill_side_kinds(fs_batch *b, int side, int kind) {
  const size_t B = b->d.n_reaches;
  const std::vector<int32_t> same(B, kind);
  return upload_i32(b->reach_kinds.get<int32_t>() + (size_t)side * B, same.data(), B);
}

// this side now holds one kind for the whole batch (where the other side has per-reach kinds, the kind goes into every slot of this one)
int set_side_kind(fs_batch *b, int side, int kind, int stride) {
  b->bc_kind[side] = kind; b->bc_stride[side] = stride;
  b->have_bc[side] = true;
  b->kinds_per_reach[side] = false; b->any_storage[side] = fs::bc_is_storage(kind); b->some_host_rows[side] = false;
  return b->reach_kinds ? fill_side_kinds(b, side, kind) : 0;
}

// the [2][B] int32 block a kernel reports per reach in: exists, row 0 zeros and row 1 all ones (-1) ...
int prepare_info(fs_batch *b, fs::DeviceBuffer &block) {
  const size_t B = b->d.n_reaches;
  HIP_TRY(block.ensure(2 * B * sizeof(int32_t)));
  HIP_TRY(hipMemsetAsync(block.get(), 0, B * sizeof(int32_t), b->stream));
  HIP_TRY(hipMemsetAsync(block.get<int32_t>() + B, 0xff, B * sizeof(int32_t), b->stream));
  return 0;
}

// ... and back to the caller who asked for it
int return_info(fs_batch *b, const fs::DeviceBuffer &block, int32_t *info) {
  if (!info) return 0;
  HIP_TRY(hipMemcpyAsync(info, block.get(), 2 * (size_t)b->d.n_reaches * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// the polylines and their tables leave the device (a new irregular geometry follows) ...
void reset_polylines(fs_batch *b) {
  for (fs::DeviceBuffer *q : {&b->geo_table, &b->poly_x, &b->poly_z, &b->poly_lim, &b->poly_tz, &b->poly_n}) q->reset();
  b->poly_K = 0;
}

// ... and n_sets channels of P stations are on it (1: shared by the batch), with stage tables or for the edge walk
void commit_polylines(fs_batch *b, size_t n_sets, size_t P, bool walk) {
  const size_t N = b->d.n_nodes;
  b->poly_K = walk ? 0 : (int)P;
  b->poly_P = (int)P;
  b->geo_reach_stride = n_sets > 1 ? (size_t)fs::FS_GEOX_NROWS * N : 0;
  b->poly_reach_stride = n_sets > 1 ? P * N : 0;
  b->have_geo = true;
}

// the state in hk / Qk becomes the Newton start vector and, where a history is kept, its level 0 (solver.py:61-63)
int spread_level0(fs_batch *b) {
  const size_t bytes = (size_t)b->d.n_reaches * b->d.n_nodes * b->esz;
  HIP_TRY(hipMemcpyAsync(b->hg.get(), b->hk.get(), bytes, hipMemcpyDeviceToDevice, b->stream));
  HIP_TRY(hipMemcpyAsync(b->Qg.get(), b->Qk.get(), bytes, hipMemcpyDeviceToDevice, b->stream));
  if (b->hist_h) {
    HIP_TRY(hipMemcpyAsync(b->hist_h.get(), b->hk.get(), bytes, hipMemcpyDeviceToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->hist_Q.get(), b->Qk.get(), bytes, hipMemcpyDeviceToDevice, b->stream));
  }
  return 0;
}

// a new initial state is on the device: the per-level records start over
int begin_at_level0(fs_batch *b) {
  const size_t B = b->d.n_reaches, L = b->d.max_levels;
  HIP_TRY(hipMemsetAsync(b->status.get(), 0, B * 4, b->stream));
  HIP_TRY(hipMemsetAsync(b->iters.get(), 0, L * B * 4, b->stream));
  HIP_TRY(hipMemsetAsync(b->Yprev.get(), 0, B * b->esz, b->stream));
  if (b->trace) HIP_TRY(hipMemsetAsync(b->trace.get(), 0, L * FS_TRACE_CAP * B * b->esz, b->stream));
  HIP_TRY(hipMemsetAsync(b->it_done.get(), 0, B * 4, b->stream));
  if (b->integ) {      // no row holds integrals of the new run
    fs::launch_clear_integrals(b->integ.get<double>(), L * FS_INT_NROWS * B, b->integ_mark.get<int32_t>(), L * B, b->stream);
    HIP_TRY(hipGetLastError());
  }
  if (b->gauge) {      // ... and no row holds a gauge's values
    fs::launch_clear_integrals(b->gauge.get<double>(), (size_t)b->n_gauges * L * FS_GAUGE_NROWS * B, b->gauge_mark.get<int32_t>(), L * B, b->stream);
    HIP_TRY(hipGetLastError());
    std::fill(b->gauge_levels.begin(), b->gauge_levels.end(), 0);
  }
  b->level = 0; b->iterating = false; b->restart_level = 0;
  b->have_state = true;
  return 0;
}

// stream, events and the buffers every batch has, on the batch's device (which stays current)
int init_batch(fs_batch *b) {
  HIP_TRY(hipSetDevice(b->d.device));
  HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&b->ev0));
  HIP_TRY(hipEventCreate(&b->ev1));
  const size_t B = b->d.n_reaches, N = b->d.n_nodes, L = b->d.max_levels, esz = b->esz;
  auto zeroed = [&](fs::DeviceBuffer &buf, size_t bytes) -> int {
    HIP_TRY(buf.ensure(bytes));
    HIP_TRY(hipMemsetAsync(buf.get(), 0, bytes, b->stream));
    return 0;
  };
  for (fs::DeviceBuffer *p : {&b->hk, &b->Qk, &b->hg, &b->Qg}) HIP_TRY(p->ensure(B * N * esz));
  if (zeroed(b->hydro, L * 4 * B * esz) || zeroed(b->iters, L * B * 4) || zeroed(b->status, B * 4) || zeroed(b->Yprev, B * esz) ||
      zeroed(b->stage_hist, L * B * esz) || zeroed(b->it_done, B * 4)) return -1;
  if ((b->d.flags & FS_FLAG_TRACE) && zeroed(b->trace, L * FS_TRACE_CAP * B * esz)) return -1;
  if (b->d.flags & FS_FLAG_HISTORY) {
    HIP_TRY(b->hist_h.ensure(L * B * N * esz));
    HIP_TRY(b->hist_Q.ensure(L * B * N * esz));
  }
#ifdef FS_STAMP
  if (zeroed(b->dbg, B * 16 * 12 * 8)) return -1;
#endif
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (B * N * esz >= kStageMin) (void)b->stage.init();        // large batch: the pinned chunks exist before the first transfer is timed
  return 0;
}


// ---- post-processing (fs_reduce.hpp, fs_envelope.hpp, fs_balance.hpp): what its entry points share; their checks and layouts are
// fs_host_post.hpp ----

// a check of fs_host_post.hpp: its text, if it has one, becomes the error
int refuse(const std::string &text) { return text.empty() ? 0 : fail(text); }

// the range [first, first + n) must hold computed rows only
int check_reduce_range(const fs_batch *b, const char *entry, int32_t first, int32_t n,
                       const char *not_restored = "the hydrograph rows before it were not restored") {
  if (!b->have_state) return fail(std::string(entry) + ": no state yet");
  return refuse(fs::check_computed_range(entry, first, n, b->level, b->restart_level, not_restored));
}

// the batch's section tables as derive, envelope and reach integrals read them
template <typename R> fs::SectionTables<R> section_tables(const fs_batch *b) {
  return fs::SectionTables<R>{b->geo_uniform.get<const R>(), b->geo_table.get<const R>(), b->poly_x.get<const R>(), b->poly_z.get<const R>(),
                              b->poly_n.get<const int32_t>(), (int64_t)b->geo_reach_stride, (int64_t)b->poly_reach_stride};
}

template <typename R> fs::ReduceArgs<R> reduce_args(const fs_batch *b, int32_t first, int32_t n) {
  return fs::ReduceArgs<R>{b->hydro.get<const R>(), b->status.get<const int32_t>(), b->iters.get<const int32_t>(), b->d.n_reaches, b->level, first, n};
}

// n doubles of the caller's into a double buffer of the handle (the batch's dtype does not apply to these)
int upload_f64(fs::DeviceBuffer &dst, const double *src, size_t n) {
  HIP_TRY(dst.reserve(n * sizeof(double)));
  HIP_TRY(hipMemcpy(dst.get(), src, n * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

int fetch(fs_batch *b, void *dst, const void *dev, size_t bytes) {
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(dst, dev, bytes, hipMemcpyDeviceToHost));
  return 0;
}

const char kNoReduceKernels[] = ": this build has no post-processing kernels";

// One post-processing launch on the handle's stream: launch(real), handed the batch's type as with_real does, says whether this build
// has the kernel.  launches > 0: the two events are recorded around it, and fs_batch_last_step_ms() / fs_batch_last_launch_count()
// then report it; 0: they keep what they held.
template <typename Launch> int post_launch(fs_batch *b, const char *entry, int launches, Launch &&launch) {
  if (launches > 0) HIP_TRY(hipEventRecord(b->ev0, b->stream));
  if (!with_real(b, launch)) return fail(std::string(entry) + kNoReduceKernels);
  HIP_TRY(hipGetLastError());
  if (launches > 0) {
    HIP_TRY(hipEventRecord(b->ev1, b->stream));
    b->timed = true; b->launches = launches;
  }
  return 0;
}

// the outputs of a band call (fs::BandArgs, fs::ProfileBandArgs) that the caller asked for, in the block at blk; q: the levels on the device
template <typename Args> void point_bands(Args &p, const fs::BandLayout &l, double *blk, const double *q, int32_t n_q, bool moments, bool members) {
  p.q = l.n_quantiles ? q : nullptr; p.n_q = l.n_quantiles ? n_q : 0;
  p.moments = moments ? blk + l.moments : nullptr; p.quantiles = l.n_quantiles ? blk + l.quantiles : nullptr;
  p.n_members = members ? (int32_t *)(blk + l.members) : nullptr;
}

// ... and back to the caller; extra: the per-series row of the layout, or nullptr
int fetch_bands(fs_batch *b, const fs::BandLayout &l, const double *blk, double *moments, double *quantiles, double *extra, int32_t *members) {
  if (moments && fetch(b, moments, blk + l.moments, l.n_moments * sizeof(double))) return -1;
  if (l.n_quantiles && fetch(b, quantiles, blk + l.quantiles, l.n_quantiles * sizeof(double))) return -1;
  if (extra && fetch(b, extra, blk + l.extra, l.series * sizeof(double))) return -1;
  if (members && fetch(b, members, blk + l.members, l.series * sizeof(int32_t))) return -1;
  return 0;
}

// ---- forcing on the device (fs_forcing.hpp) ----

// the per-reach time steps in fp64 for the forcing kernels (nullptr: the batch's dt)
int forcing_reach_dt(fs_batch *b, const double **out) {
  *out = nullptr;
  if (b->rs_host[1].empty()) { b->frc_dt.reset(); return 0; }
  if (upload_f64(b->frc_dt, b->rs_host[1].data(), b->rs_host[1].size())) return -1;
  *out = b->frc_dt.get<const double>();
  return 0;
}

}  // namespace

extern "C" {

int fs_abi_version(void) { return FS_ABI_VERSION; }

int fs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *fs_last_error(void) { return g_err.c_str(); }

fs_batch *fs_batch_create(const fs_batch_desc *desc) {
  if (!desc) { fail("fs_batch_create: null descriptor"); return nullptr; }
  if (desc->n_reaches < 1 || desc->n_nodes < 2 || desc->max_levels < 2) {
    fail("fs_batch_create: need n_reaches >= 1, n_nodes >= 2, max_levels >= 2"); return nullptr;
  }
  if (desc->dtype != FS_F64 && desc->dtype != FS_F32) { fail("fs_batch_create: bad dtype"); return nullptr; }
  if (!fs::sec_is_uniform(desc->section_mode) && !fs::sec_has_tables(desc->section_mode)) {
    fail("fs_batch_create: bad section_mode"); return nullptr;
  }
  if (desc->section_mode == FS_SEC_IRREGULAR && desc->dtype != FS_F64) {
    fail("fs_batch_create: FS_SEC_IRREGULAR is fp64 only"); return nullptr;
  }
  if (fs_device_count() <= desc->device || desc->device < 0) {
    fail("fs_batch_create: no HIP device " + std::to_string(desc->device) +
         " (this library has no CPU path; it needs an MI355X)");
    return nullptr;
  }
  std::string why;
  // a first choice, before the boundary kinds are known: is there a kernel for this size at all?  (FS_KERNEL_INDEX is for the steps.)
  fs::Query q;
  q.dtype = desc->dtype; q.sec = desc->section_mode; q.N = desc->n_nodes; q.usk = q.dsk = FS_BC_FLOW_HYDROGRAPH; q.need_diag = true;
  fs::Overrides ov = fs::overrides_from_environment();
  ov.force_index = false;
  const int chosen = fs::pick(kEntries, kNumEntries, q, ov, &why);
  if (chosen < 0) { fail("fs_batch_create: " + why); return nullptr; }
  fs_batch *b = new fs_batch();
  b->d = *desc;
  b->esz = desc->dtype == FS_F64 ? 8 : 4;
  b->kern = &kEntries[chosen];
  int prev_dev = -1;
  if (hipGetDevice(&prev_dev) != hipSuccess) prev_dev = -1;
  if (init_batch(b)) {
    const std::string what = g_err;
    fs_batch_destroy(b);
    b = nullptr;
    fail("fs_batch_create: " + what);
  }
  if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
  return b;
}

// (the buffers go while the stream and the events still exist: fs_batch's members before its base, Timeline)
void fs_batch_destroy(fs_batch *b) {
  if (!b) return;
  DeviceGuard guard_(b->d.device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  delete b;
}

static int rebuild_reach_scheme(fs_batch *b);

int fs_batch_set_scheme(fs_batch *b, double theta, double dt, double dx, double tolerance, int32_t max_iter) {
  if (!b) return fail("null handle");
  if (!(dt > 0) || !(dx > 0) || !(tolerance > 0) || max_iter < 1) return fail("fs_batch_set_scheme: dt, dx, tolerance > 0 and max_iter >= 1 required");
  b->theta = theta; b->dt = dt; b->dx = dx; b->tol = tolerance; b->max_iter = max_iter;
  b->have_scheme = true; b->bal_scheme_stale = true;
  if (b->reach_scheme) {      // per-reach values stand; the rows the caller left to the batch take the new numbers
    FS_ON_DEVICE(b);
    return rebuild_reach_scheme(b);
  }
  return 0;
}

int fs_batch_set_geometry_uniform(fs_batch *b, const double *params) {
  if (!b || !params) return fail("fs_batch_set_geometry_uniform: null argument");
  const bool trap = b->d.section_mode == FS_SEC_TRAP_UNIFORM;
  FS_ON_DEVICE(b);
  if (b->d.section_mode != FS_SEC_RECT_UNIFORM && !trap) return fail("fs_batch_set_geometry_uniform: batch was created with another section_mode");
  const size_t B = b->d.n_reaches;
  for (size_t i = 0; i < B; ++i) {
    if (!(params[FS_RU_WIDTH * B + i] > 0) || !(params[FS_RU_MANNING * B + i] > 0))
      return fail("fs_batch_set_geometry_uniform: width and Manning n must be positive");
    if (trap && !(params[FS_TU_SIDE_SLOPE * B + i] >= 0)) return fail("fs_batch_set_geometry_uniform: side slope must be >= 0");
  }
  if (upload(b, b->geo_uniform, params, (size_t)(trap ? FS_TU_NPARAM : FS_RU_NPARAM) * B)) return -1;
  b->have_geo = true;
  return 0;
}

int fs_batch_set_geometry_table(fs_batch *b, const double *table, const double *n_main_override) {
  if (!b || !table) return fail("fs_batch_set_geometry_table: null argument");
  if (b->d.section_mode != FS_SEC_TABLE) return fail("fs_batch_set_geometry_table: batch was created with another section_mode");
  FS_ON_DEVICE(b);
  const std::vector<double> x = fs::extend_table(table, b->d.n_nodes);
  b->geo_reach_stride = 0;
  if (upload(b, b->geo_table, x.data(), x.size()) || set_n_override(b, n_main_override)) return -1;
  b->have_geo = true;
  return 0;
}

// n_sets = 1: one channel shared by the batch; n_sets = B: one per reach (tables [B][NPARAM][N], n_pts [B][N], x / z [B][N][P],
// limits [B][N][2]).  What goes to the device, and whether with stage tables: fs::plan_irregular
static int set_irregular(fs_batch *b, const double *table, const int32_t *n_pts, int32_t max_pts, const double *x, const double *z,
                         const double *limits, const double *n_main_override, size_t n_sets) {
  if (!b || !table || !n_pts || !x || !z || !limits) return fail("fs_batch_set_geometry_irregular: null argument");
  if (b->d.section_mode != FS_SEC_IRREGULAR) return fail("fs_batch_set_geometry_irregular: batch was created with another section_mode");
  if (max_pts < 2) return fail("fs_batch_set_geometry_irregular: max_pts must be >= 2");
  FS_ON_DEVICE(b);
  const size_t N = b->d.n_nodes, P = max_pts;
  fs::IrregularPlan plan;
  const std::string err = fs::plan_irregular(table, n_pts, max_pts, x, z, limits, N, n_sets, fs::poly_limits_from_environment(), plan);
  if (!err.empty()) return fail(err);
  reset_polylines(b);
  if (!plan.walk && upload(b, b->poly_tz, plan.tz.data(), plan.tz.size()))
    return fail("fs_batch_set_geometry_irregular: " + std::to_string(plan.table_mib) + " MiB of stage tables do not fit the "
                "device (" + g_err + "); lower FS_POLY_TABLE_MAX_BYTES to fall back to the edge walk");
  if (upload(b, b->geo_table, plan.tabs.data(), plan.tabs.size()) || upload(b, b->poly_x, plan.xt.data(), plan.xt.size()) ||
      upload(b, b->poly_z, plan.zt.data(), plan.zt.size()) || upload(b, b->poly_lim, plan.lim.data(), plan.lim.size())) return -1;
  HIP_TRY(b->poly_n.ensure(n_sets * N * sizeof(int32_t)));
  if (upload_i32(b->poly_n.get<int32_t>(), n_pts, n_sets * N) || set_n_override(b, n_main_override)) return -1;
  commit_polylines(b, n_sets, P, plan.walk);
  return 0;
}

int fs_batch_set_geometry_irregular(fs_batch *b, const double *table, const int32_t *n_pts, int32_t max_pts,
                                    const double *x, const double *z, const double *limits,
                                    const double *n_main_override) {
  return set_irregular(b, table, n_pts, max_pts, x, z, limits, n_main_override, 1);
}

int fs_batch_set_geometry_irregular_per_reach(fs_batch *b, const double *tables, const int32_t *n_pts, int32_t max_pts,
                                              const double *x, const double *z, const double *limits,
                                              const double *n_main_override) {
  if (!b) return fail("fs_batch_set_geometry_irregular: null argument");
  return set_irregular(b, tables, n_pts, max_pts, x, z, limits, n_main_override, (size_t)b->d.n_reaches);
}

// One surveyed channel and per-member transforms: the members' polylines, tables and stage tables are built on the device
// (fs_member_geo.hpp); only the shared channel and the transforms cross the bus.
int fs_batch_set_geometry_irregular_members(fs_batch *b, const double *table, const int32_t *n_pts, int32_t max_pts, const double *x,
                                            const double *z, const double *limits, const double *dz_left, const double *dz_main,
                                            const double *dz_right, const double *n_scale) {
  if (!b || !table || !n_pts || !x || !z || !limits) return fail("fs_batch_set_geometry_irregular_members: null argument");
  if (b->d.section_mode != FS_SEC_IRREGULAR) return fail("fs_batch_set_geometry_irregular_members: batch was created with another section_mode");
  if (max_pts < 2) return fail("fs_batch_set_geometry_irregular: max_pts must be >= 2");
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches, N = b->d.n_nodes, P = max_pts;
  if (const char *err = fs::check_member_transforms(n_pts, dz_left, dz_main, dz_right, n_scale, B, N)) return fail(err);
  // the shared channel through the validation and the transposition of the other irregular setters, without the tables
  std::vector<double> xt(P * N), zt(P * N), lim(2 * N);
  if (const char *err = fs::pack_polylines(table, n_pts, max_pts, x, z, limits, N, xt.data(), zt.data(), lim.data(), nullptr)) return fail(err);
  const std::vector<double> ext = fs::extend_table(table, N);
  size_t table_mib;
  const bool walk = fs::poly_tables_walk(B, N, max_pts, fs::poly_limits_from_environment(), &table_mib);
  reset_polylines(b);
  b->poly_P = 0; b->have_geo = false;
  if (!walk && b->poly_tz.ensure(B * N * fs::poly_table_stride(max_pts) * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    return fail("fs_batch_set_geometry_irregular_members: " + std::to_string(table_mib) + " MiB of stage tables do not "
                "fit the device; lower FS_POLY_TABLE_MAX_BYTES to fall back to the edge walk");
  }
  HIP_TRY(b->geo_table.ensure(B * fs::FS_GEOX_NROWS * N * sizeof(double)));
  HIP_TRY(b->poly_x.ensure(B * P * N * sizeof(double)));
  HIP_TRY(b->poly_z.ensure(B * P * N * sizeof(double)));
  HIP_TRY(b->poly_lim.ensure(B * 2 * N * sizeof(double)));
  HIP_TRY(b->poly_n.ensure(B * N * sizeof(int32_t)));
  fs::DeviceBuffer *in = b->member_in;
  if (upload_f64(in[0], xt.data(), xt.size()) || upload_f64(in[1], zt.data(), zt.size()) || upload_f64(in[2], lim.data(), lim.size()) ||
      upload_f64(in[4], ext.data(), ext.size())) return -1;
  HIP_TRY(in[3].reserve(N * sizeof(int32_t)));
  if (upload_i32(in[3].get<int32_t>(), n_pts, N)) return -1;
  const double *opt[4] = {dz_left, dz_main, dz_right, n_scale};
  for (int q = 0; q < 4; ++q)
    if (opt[q] && upload_f64(in[5 + q], opt[q], q < 3 ? B * N : 3 * B)) return -1;
  auto given = [&](int q) { return opt[q] ? in[5 + q].get<const double>() : nullptr; };
  fs::MemberGeoArgs a{in[0].get<const double>(), in[1].get<const double>(), in[2].get<const double>(), in[3].get<const int32_t>(),
                      in[4].get<const double>(), {given(0), given(1), given(2)}, given(3),
                      b->poly_x.get<double>(), b->poly_z.get<double>(), b->poly_lim.get<double>(), b->poly_n.get<int32_t>(),
                      b->geo_table.get<double>(), b->poly_tz.get<double>(), (int64_t)B, (int64_t)N, max_pts};
  {
    TraceRange range_("flowsim:member_geometry");
    HIP_TRY(hipEventRecord(b->ev0, b->stream));
    if (!fs::launch_member_sections(a, b->stream) || (!walk && !fs::launch_member_tables(a, b->stream)))
      return fail("fs_batch_set_geometry_irregular_members: this build has no geometry kernels");
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->ev1, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->timed = true; b->launches = walk ? 1 : 2;      // fs_batch_last_step_ms: the two kernels, until the next step
  }
  b->n_override.reset();      // n_scale[1] takes its place
  commit_polylines(b, B, P, walk);
  return 0;
}

// One TrapezoidalSection table per reach: tables[B][FS_GEO_NPARAM][N] on the host -> [B][FS_GEOX_NROWS][N] on the device (a
// reach's workgroup reads its own table, lanes along the nodes: coalesced; once per launch in the two-rows-per-lane kernels)
int fs_batch_set_geometry_table_per_reach(fs_batch *b, const double *tables, const double *n_main_override) {
  if (!b || !tables) return fail("fs_batch_set_geometry_table_per_reach: null argument");
  if (b->d.section_mode != FS_SEC_TABLE) return fail("fs_batch_set_geometry_table_per_reach: batch was created with another section_mode");
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches, N = b->d.n_nodes, per = (size_t)fs::FS_GEOX_NROWS * N;
  std::vector<double> all(B * per);
  for (size_t r = 0; r < B; ++r) {
    const std::vector<double> x = fs::extend_table(tables + r * FS_GEO_NPARAM * N, N);
    std::memcpy(all.data() + r * per, x.data(), per * sizeof(double));
  }
  if (upload(b, b->geo_table, all.data(), all.size())) return -1;
  b->geo_reach_stride = per;
  if (set_n_override(b, n_main_override)) return -1;
  b->have_geo = true;
  return 0;
}

int fs_batch_set_reach_nodes(fs_batch *b, const int32_t *n_nodes) {
  if (!b) return fail("null handle");
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches;
  // the level-0 hydrograph row holds each reach's LAST node (fs_batch_set_state): when the counts change under a state that is
  // already on the device and has not been stepped, the row follows them
  auto refresh_row0 = [&]() -> int {
    if (!b->have_state || b->level != 0) return 0;
    with_real(b, [&](auto real) {
      using R = decltype(real);
      hipLaunchKernelGGL((refresh_level0_downstream<R>), grid_256(B), dim3(256), 0, b->stream, b->hk.get<const R>(), b->Qk.get<const R>(),
                         b->reach_nodes.get<const int32_t>(), b->hydro.get<R>(), B, (size_t)b->d.n_nodes);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
  };
  if (!n_nodes) {
    b->reach_nodes.reset();
    b->reach_nodes_host.clear();
    return refresh_row0();
  }
  for (size_t r = 0; r < B; ++r)
    if (n_nodes[r] < 2 || n_nodes[r] > b->d.n_nodes) return fail("fs_batch_set_reach_nodes: every reach needs 2 <= nodes <= n_nodes of the batch");
  HIP_TRY(b->reach_nodes.ensure(B * sizeof(int32_t)));
  if (upload_i32(b->reach_nodes.get<int32_t>(), n_nodes, B)) return -1;
  b->reach_nodes_host.assign(n_nodes, n_nodes + B);
  return refresh_row0();
}

// the [5][B] array of per-reach scheme values (fs::merge_reach_scheme) on the device, or none
static int rebuild_reach_scheme(fs_batch *b) {
  const double wide[5] = {b->theta, b->dt, b->dx, b->tol, (double)b->max_iter};
  const std::vector<double> v = fs::merge_reach_scheme(b->rs_host, wide, b->d.n_reaches);
  b->reach_scheme.reset();
  return v.empty() ? 0 : upload(b, b->reach_scheme, v.data(), v.size());
}

int fs_batch_set_reach_scheme(fs_batch *b, const double *theta, const double *dt, const double *dx) {
  if (!b) return fail("null handle");
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches;
  if ((theta || dt || dx) && !b->have_scheme)
    return fail("fs_batch_set_reach_scheme: call fs_batch_set_scheme first (tolerance, max_iter and the values of the arrays left NULL)");
  for (size_t r = 0; r < B; ++r)
    if ((dt && !(dt[r] > 0)) || (dx && !(dx[r] > 0))) return fail("fs_batch_set_reach_scheme: dt and dx must be positive");
  const double *src[3] = {theta, dt, dx};
  for (int i = 0; i < 3; ++i) {
    if (src[i]) b->rs_host[i].assign(src[i], src[i] + B); else b->rs_host[i].clear();
  }
  b->bal_scheme_stale = true;
  return rebuild_reach_scheme(b);
}

int fs_batch_set_reach_tolerance(fs_batch *b, const double *tolerance, const int32_t *max_iter) {
  if (!b) return fail("null handle");
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches;
  if ((tolerance || max_iter) && !b->have_scheme) return fail("fs_batch_set_reach_tolerance: call fs_batch_set_scheme first");
  for (size_t r = 0; r < B; ++r)
    if ((tolerance && !(tolerance[r] > 0)) || (max_iter && max_iter[r] < 1)) return fail("fs_batch_set_reach_tolerance: tolerance > 0 and max_iter >= 1 required");
  if (tolerance) b->rs_host[3].assign(tolerance, tolerance + B); else b->rs_host[3].clear();
  if (max_iter) b->rs_host[4].assign(max_iter, max_iter + B); else b->rs_host[4].clear();
  return rebuild_reach_scheme(b);
}

int fs_batch_set_bc_per_reach(fs_batch *b, int32_t side, const int32_t *kinds, const double *params, const double *target) {
  return fs_batch_set_bc_per_reach_wide(b, side, kinds, params, FS_BC_MAX_PARAMS, target);
}

int fs_batch_set_bc_per_reach_wide(fs_batch *b, int32_t side, const int32_t *kinds, const double *params, int32_t n_params,
                                   const double *target) {
  if (!b || !kinds || !params) return fail("fs_batch_set_bc_per_reach: null argument");
  if (check_side("fs_batch_set_bc_per_reach", side)) return -1;
  if (n_params < FS_BC_MAX_PARAMS) return fail("fs_batch_set_bc_per_reach: at least FS_BC_MAX_PARAMS parameter rows");
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches;
  fs::SideKinds sk;
  if (const char *err = fs::check_bc_per_reach(side, kinds, params, n_params, target != nullptr, B, fs::sec_has_tables(b->d.section_mode), sk))
    return fail(err);
  if (replace_bc_buffers(b, side, params, (size_t)n_params * B, target)) return -1;
  if (!b->reach_kinds) {
    HIP_TRY(b->reach_kinds.ensure(2 * B * 4));
    HIP_TRY(hipMemset(b->reach_kinds.get(), 0, 2 * B * 4));
  }
  if (upload_i32(b->reach_kinds.get<int32_t>() + (size_t)side * B, kinds, B)) return -1;
  // the other side, if it was set for the whole batch, keeps its one kind in every slot
  const int other = 1 - side;
  if (b->have_bc[other] && !b->kinds_per_reach[other] && fill_side_kinds(b, other, b->bc_kind[other])) return -1;
  b->bc_kind[side] = sk.kind; b->bc_stride[side] = 1; b->kinds_per_reach[side] = true;
  b->any_storage[side] = sk.any_storage; b->some_host_rows[side] = sk.some_host_rows;
  b->have_bc[side] = true;
  return 0;
}

int fs_batch_set_bc(fs_batch *b, int32_t side, int32_t kind, const double *params, int32_t n_params,
                    int32_t per_reach, const double *target) {
  if (!b) return fail("null handle");
  if (check_side("fs_batch_set_bc", side)) return -1;
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches;
  if (const char *err = fs::check_bc(side, kind, params, n_params, per_reach, target != nullptr, B, fs::sec_has_tables(b->d.section_mode)))
    return fail(err);
  if (kind == FS_BC_HOST_ROW) {      // params[3][B], or NULL: zeros until fs_batch_set_host_rows
    if (replace_bc_buffers(b, side, params, 3 * B, nullptr)) return -1;
  } else if (replace_bc_buffers(b, side, params, per_reach ? n_params * B : (size_t)n_params, target)) return -1;
  return set_side_kind(b, side, kind, (kind == FS_BC_HOST_ROW || per_reach) ? 1 : 0);
}

int fs_batch_set_state(fs_batch *b, const double *h, const double *Q) {
  if (!b || !h || !Q) return fail("fs_batch_set_state: null argument");
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches, N = b->d.n_nodes;
  // each array crosses the bus once; the Newton start vector and level 0 of the history are device-to-device copies
  if (upload(b, b->hk, h, B * N) || upload(b, b->Qk, Q, B * N)) return -1;
  if (spread_level0(b)) return -1;
  std::vector<double> row(4 * B);
  for (size_t r = 0; r < B; ++r) {
    const size_t last = (b->reach_nodes_host.empty() ? N : (size_t)b->reach_nodes_host[r]) - 1;     // the reach's own last node, not the caller's padding
    row[0 * B + r] = h[r * N]; row[1 * B + r] = Q[r * N];
    row[2 * B + r] = h[r * N + last]; row[3 * B + r] = Q[r * N + last];
  }
  if (upload_to(b, b->hydro.get(), row.data(), 4 * B)) return -1;
  return begin_at_level0(b);
}

int fs_batch_set_state_uniform(fs_batch *b, const double *h, const double *Q) {
  if (!b || !h || !Q) return fail("fs_batch_set_state_uniform: null argument");
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches, N = b->d.n_nodes;
  fs::DeviceBuffer dh, dQ;
  if (upload(b, dh, h, B) || upload(b, dQ, Q, B)) return -1;
  with_real(b, [&](auto real) {
    using R = decltype(real);
    hipLaunchKernelGGL((broadcast_state<R>), grid_256(B * N), dim3(256), 0, b->stream, dh.get<const R>(), dQ.get<const R>(), b->hk.get<R>(),
                       b->Qk.get<R>(), b->hg.get<R>(), b->Qg.get<R>(), b->hist_h.get<R>(), b->hist_Q.get<R>(), b->hydro.get<R>(), B, N);
  });
  HIP_TRY(hipGetLastError());
  if (begin_at_level0(b)) return -1;
  HIP_TRY(hipStreamSynchronize(b->stream));      // (dh and dQ go when this returns)
  return 0;
}

int fs_batch_init_state(fs_batch *b, int32_t method, const double *flow, const double *depth_us, const double *depth_ds,
                        const double *bed_slope, int32_t bed_slope_per_reach, int32_t *info) {
  if (!b || !flow) return fail("fs_batch_init_state: null argument");
  if (method != FS_IC_LINEAR && method != FS_IC_GVF && method != FS_IC_STEADY)
    return fail("fs_batch_init_state: method must be FS_IC_LINEAR, FS_IC_GVF or FS_IC_STEADY");
  if (!b->have_scheme || !b->have_geo)
    return fail(std::string("fs_batch_init_state: ") + (!b->have_scheme ? (!b->have_geo ? "the scheme (fs_batch_set_scheme: dx) and the geometry" : "the scheme (fs_batch_set_scheme: dx)") : "the geometry") +
                " must be set first");
  if (method != FS_IC_STEADY && !depth_ds) return fail("fs_batch_init_state: depth_ds is needed by FS_IC_LINEAR and FS_IC_GVF");
  if (method == FS_IC_LINEAR && !depth_us) return fail("fs_batch_init_state: depth_us is needed by FS_IC_LINEAR");
  const size_t B = b->d.n_reaches, N = b->d.n_nodes;
  if (method == FS_IC_STEADY) {
    if (!bed_slope && !fs::sec_is_uniform(b->d.section_mode)) return fail("fs_batch_init_state: FS_IC_STEADY needs bed_slope in section modes FS_SEC_TABLE and FS_SEC_IRREGULAR");
    if (bed_slope)        // the reference's None (channel.py:299-300), at a reach's own nodes
      for (size_t r = 0; r < (bed_slope_per_reach ? B : 1); ++r) {
        size_t n_r = N;
        if (bed_slope_per_reach && !b->reach_nodes_host.empty()) n_r = (size_t)b->reach_nodes_host[r];
        for (size_t i = 0; i < n_r; ++i)
          if (std::isnan(bed_slope[r * N + i])) return fail("fs_batch_init_state: Bed slope must be defined.");
      }
  }
  FS_ON_DEVICE(b);
  // (the batch keeps the inputs: the kernels read them after this call has returned)
  fs::DeviceBuffer &d_flow = b->ic_in[0], &d_us = b->ic_in[1], &d_ds = b->ic_in[2], &d_slope = b->ic_in[3];
  HIP_TRY(hipStreamSynchronize(b->stream));      // an earlier call's kernels are through with them
  if (method != FS_IC_LINEAR) d_us.reset();      // (what this method does not read must read as "not given")
  if (method == FS_IC_STEADY) d_ds.reset();
  if (method != FS_IC_STEADY || !bed_slope) d_slope.reset();
  if (upload(b, d_flow, flow, B)) return -1;
  if (method == FS_IC_LINEAR && upload(b, d_us, depth_us, B)) return -1;
  if (method != FS_IC_STEADY && upload(b, d_ds, depth_ds, B)) return -1;
  if (method == FS_IC_STEADY && bed_slope && upload(b, d_slope, bed_slope, bed_slope_per_reach ? B * N : N)) return -1;
  if (prepare_info(b, b->ic_info)) return -1;
  {
    TraceRange range_("flowsim:init_state");
    const bool launched = with_real(b, [&](auto real) {
      using R = decltype(real);
      fs::InitArgs<R> p;
      fill_args(b, 0, p.k);
      p.method = method; p.flow = d_flow.get<const R>(); p.depth_us = d_us.get<const R>(); p.depth_ds = d_ds.get<const R>();
      p.bed_slope = d_slope.get<const R>(); p.bed_slope_per_reach = bed_slope_per_reach; p.info = b->ic_info.get<int32_t>();
      const bool ok = fs::launch_init_state(b->d.section_mode, p, b->stream);
      if (ok) {      // the level-0 hydrograph row: node 0 and each reach's own last node
        hipLaunchKernelGGL((refresh_level0_upstream<R>), grid_256(B), dim3(256), 0, b->stream, b->hk.get<const R>(), b->Qk.get<const R>(), b->hydro.get<R>(), B, N);
        hipLaunchKernelGGL((refresh_level0_downstream<R>), grid_256(B), dim3(256), 0, b->stream, b->hk.get<const R>(), b->Qk.get<const R>(),
                           b->reach_nodes.get<const int32_t>(), b->hydro.get<R>(), B, N);
      }
      return ok;
    });
    if (!launched) return fail("fs_batch_init_state: this build has no initial-condition kernel for this section mode and dtype");
    HIP_TRY(hipGetLastError());
  }
  if (spread_level0(b) || begin_at_level0(b)) return -1;
  return return_info(b, b->ic_info, info);
}

int fs_batch_set_bc_sampled(fs_batch *b, int32_t side, int32_t kind, const double *params, int32_t n_params, const double *times,
                            const double *values, int32_t n_pts, int32_t n_tables, const int32_t *table_of, const double *scale,
                            const double *offset, const double *shift) {
  if (!b) return fail("fs_batch_set_bc_sampled: null handle");
  if (check_side("fs_batch_set_bc_sampled", side)) return -1;
  if (kind != FS_BC_FLOW_HYDROGRAPH && kind != FS_BC_STAGE_HYDROGRAPH)
    return fail("fs_batch_set_bc_sampled: kind must be FS_BC_FLOW_HYDROGRAPH or FS_BC_STAGE_HYDROGRAPH");
  if (!b->have_scheme) return fail("fs_batch_set_bc_sampled: the scheme (fs_batch_set_scheme: dt) must be set first");
  const size_t B = b->d.n_reaches, L = b->d.max_levels;
  if (const char *err = fs::check_bc(side, kind, params, n_params, 0, true, B, fs::sec_has_tables(b->d.section_mode))) return fail(err);
  if (const char *err = fs::check_sampled_tables(times, values, n_pts, n_tables, table_of, B)) return fail(err);
  FS_ON_DEVICE(b);
  HIP_TRY(hipStreamSynchronize(b->stream));      // an earlier call's kernels are through with the inputs
  b->have_bc[side] = false;                      // (until the target is filled: a failure below leaves the side unset, not half set)
  if (replace_bc_buffers(b, side, params, (size_t)n_params, nullptr)) return -1;
  HIP_TRY(b->bc_target[side].ensure(L * B * b->esz));
  fs::DeviceBuffer *in = b->frc_in[side];
  if (upload_f64(in[0], times, (size_t)n_pts) || upload_f64(in[1], values, (size_t)n_tables * n_pts)) return -1;
  if (table_of) {
    HIP_TRY(in[2].reserve(B * sizeof(int32_t)));
    if (upload_i32(in[2].get<int32_t>(), table_of, B)) return -1;
  }
  const double *per[3] = {scale, offset, shift};
  for (int i = 0; i < 3; ++i)
    if (per[i] && upload_f64(in[3 + i], per[i], B)) return -1;
  const double *reach_dt;
  if (forcing_reach_dt(b, &reach_dt)) return -1;
  {
    TraceRange range_("flowsim:forcing");
    const bool launched = with_real(b, [&](auto real) {
      using R = decltype(real);
      fs::SampleArgs<R> a;
      a.target = b->bc_target[side].get<R>(); a.L = (int32_t)L; a.B = (int32_t)B; a.n_pts = n_pts; a.n_tables = n_tables;
      a.times = in[0].get<const double>(); a.values = in[1].get<const double>();
      a.table_of = table_of ? in[2].get<const int32_t>() : nullptr;
      a.scale = scale ? in[3].get<const double>() : nullptr; a.offset = offset ? in[4].get<const double>() : nullptr;
      a.shift = shift ? in[5].get<const double>() : nullptr;
      a.reach_dt = reach_dt; a.dt = b->dt;
      return fs::launch_sample_target(a, b->stream);
    });
    if (!launched) return fail("fs_batch_set_bc_sampled: this build has no forcing kernels");
    HIP_TRY(hipGetLastError());
  }
  return set_side_kind(b, side, kind, 0);
}

int fs_batch_route_pool(fs_batch *b, int32_t side, const double *curve_stage, const double *curve_volume, int32_t n_curve,
                        const double *weirs, int32_t n_w, double base_flow, double vol_scale, double z_lo, double z_hi,
                        const double *initial_stage, const double *weir_scale, int32_t *info) {
  if (!b) return fail("fs_batch_route_pool: null handle");
  if (check_side("fs_batch_route_pool", side)) return -1;
  if (!initial_stage) return fail("fs_batch_route_pool: null initial_stage");
  if (const char *err = fs::check_pool(curve_stage, curve_volume, n_curve, weirs, n_w, base_flow, vol_scale, z_lo, z_hi)) return fail(err);
  if (!b->have_bc[side] || b->kinds_per_reach[side] || b->bc_kind[side] != FS_BC_FLOW_HYDROGRAPH || !b->bc_target[side])
    return fail("fs_batch_route_pool: this side must be an FS_BC_FLOW_HYDROGRAPH boundary of the whole batch with its target set "
                "(fs_batch_set_bc or fs_batch_set_bc_sampled): the target is the pool's inflow");
  const size_t B = b->d.n_reaches, L = b->d.max_levels;
  for (size_t r = 0; r < B; ++r)
    if (!(initial_stage[r] == initial_stage[r])) return fail("fs_batch_route_pool: initial_stage must be numbers");
  FS_ON_DEVICE(b);
  HIP_TRY(hipStreamSynchronize(b->stream));      // an earlier call's kernels are through with the inputs
  fs::DeviceBuffer *in = b->pool_in;
  if (upload_f64(in[0], curve_stage, (size_t)n_curve) || upload_f64(in[1], curve_volume, (size_t)n_curve)) return -1;
  if (n_w > 0 && upload_f64(in[2], weirs, (size_t)n_w * 4)) return -1;
  if (upload_f64(in[3], initial_stage, B)) return -1;
  if (weir_scale && n_w > 0 && upload_f64(in[4], weir_scale, (size_t)n_w * B)) return -1;
  const double *reach_dt;
  if (forcing_reach_dt(b, &reach_dt)) return -1;
  HIP_TRY(b->pool_stage.ensure(L * B * sizeof(double)));
  if (prepare_info(b, b->pool_info)) return -1;
  {
    TraceRange range_("flowsim:forcing");
    const bool launched = with_real(b, [&](auto real) {
      using R = decltype(real);
      fs::PoolArgs<R> a;
      a.target = b->bc_target[side].get<R>(); a.stage = b->pool_stage.get<double>(); a.info = b->pool_info.get<int32_t>();
      a.L = (int32_t)L; a.B = (int32_t)B; a.n_curve = n_curve; a.n_w = n_w;
      a.curve_stage = in[0].get<const double>(); a.curve_volume = in[1].get<const double>();
      a.weirs = n_w > 0 ? in[2].get<const double>() : nullptr;
      a.weir_scale = (weir_scale && n_w > 0) ? in[4].get<const double>() : nullptr;
      a.initial_stage = in[3].get<const double>(); a.reach_dt = reach_dt;
      a.dt = b->dt; a.base_flow = base_flow; a.vol_scale = vol_scale; a.z_lo = z_lo; a.z_hi = z_hi;
      return fs::launch_route_pool(a, b->stream);
    });
    if (!launched) return fail("fs_batch_route_pool: this build has no forcing kernels");
    HIP_TRY(hipGetLastError());
  }
  return return_info(b, b->pool_info, info);
}

int fs_batch_get_bc_target(fs_batch *b, int32_t side, int32_t first, int32_t n, double *out) {
  if (!b || !out) return fail("fs_batch_get_bc_target: null argument");
  if (check_side("fs_batch_get_bc_target", side)) return -1;
  if (!b->have_bc[side] || !b->bc_target[side]) return fail("fs_batch_get_bc_target: this side has no target");
  FS_ON_DEVICE(b);
  if (check_levels(b, "fs_batch_get_bc_target", first, n)) return -1;
  const size_t B = b->d.n_reaches;
  return download(b, out, b->bc_target[side], (size_t)first * B, (size_t)n * B);
}

int fs_batch_get_pool_stages(fs_batch *b, int32_t first, int32_t n, double *out) {
  if (!b || !out) return fail("fs_batch_get_pool_stages: null argument");
  if (!b->pool_stage) return fail("fs_batch_get_pool_stages: no pool has been routed on this batch");
  FS_ON_DEVICE(b);
  if (check_levels(b, "fs_batch_get_pool_stages", first, n)) return -1;
  const size_t B = b->d.n_reaches;
  return fetch(b, out, b->pool_stage.get<const double>() + (size_t)first * B, (size_t)n * B * sizeof(double));
}

int fs_batch_step(fs_batch *b, int32_t n_steps) {
  if (!b) return fail("null handle");
  if (check_ready(b, "fs_batch_step")) return -1;
  if (n_steps < 1) return fail("fs_batch_step: n_steps must be >= 1");
  if (b->level + n_steps >= b->d.max_levels) return fail("fs_batch_step: would run past max_levels");
  if (b->bc_kind[0] == FS_BC_HOST_ROW || b->bc_kind[1] == FS_BC_HOST_ROW)
    return fail("fs_batch_step: a batch with FS_BC_HOST_ROW boundaries advances with fs_batch_iterate (the caller evaluates the rows "
                "before every Newton iteration)");
  if (b->iterating) return fail("fs_batch_step: a level opened with fs_batch_iterate must be closed with it first");
  FS_ON_DEVICE(b);
  if (launch_steps(b, n_steps, 0)) return -1;
  b->level += n_steps;
  return 0;
}

int fs_batch_iterate(fs_batch *b, int32_t *n_open) {
  if (!b) return fail("null handle");
  if (check_ready(b, "fs_batch_iterate")) return -1;
  if (b->level + 1 >= b->d.max_levels) return fail("fs_batch_iterate: would run past max_levels");
  if (!fs::sec_has_tables(b->d.section_mode))
    return fail("fs_batch_iterate: section mode FS_SEC_TABLE or FS_SEC_IRREGULAR required");
  FS_ON_DEVICE(b);
  if (launch_steps(b, 1, 1)) return -1;
  b->iterating = true;
  // how many reaches are still open: counted on the device, four bytes come back
  const size_t B = b->d.n_reaches;
  HIP_TRY(b->open_dev.ensure(sizeof(int32_t)));
  HIP_TRY(b->open_pin.ensure(sizeof(int32_t)));
  HIP_TRY(hipMemsetAsync(b->open_dev.get(), 0, sizeof(int32_t), b->stream));
  hipLaunchKernelGGL(count_open_reaches, grid_256(B), dim3(256), 0, b->stream, b->it_done.get<const int32_t>(), b->status.get<const int32_t>(),
                     b->open_dev.get<int32_t>(), B);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(b->open_pin.get(), b->open_dev.get(), sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  const int32_t open = *b->open_pin.get<int32_t>();
  if (open == 0) {      // every reach has accepted the level (or failed on it): next level, counters back to zero
    b->level += 1;
    b->iterating = false;
    HIP_TRY(hipMemsetAsync(b->it_done.get(), 0, B * 4, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
  }
  if (n_open) *n_open = open;
  return 0;
}

int fs_batch_set_host_rows(fs_batch *b, int32_t side, const double *rows) {
  if (!b || !rows) return fail("fs_batch_set_host_rows: null argument");
  if (check_side("fs_batch_set_host_rows", side)) return -1;
  if (!b->have_bc[side] || b->bc_kind[side] != FS_BC_HOST_ROW) return fail("fs_batch_set_host_rows: this side is not an FS_BC_HOST_ROW boundary");
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches;
  if (!b->kinds_per_reach[side]) return upload(b, b->bc_params[side], rows, 3 * B);
  // per-reach kinds: entries of reaches whose boundary the device evaluates are ignored
  if (upload(b, b->rows_stage, rows, 3 * B)) return -1;
  with_real(b, [&](auto real) {
    using R = decltype(real);
    hipLaunchKernelGGL((merge_host_rows<R>), grid_256(B), dim3(256), 0, b->stream, b->bc_params[side].get<R>(), b->rows_stage.get<const R>(),
                       b->reach_kinds.get<const int32_t>() + (size_t)side * B, B);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

int fs_batch_get_boundary_iterate(fs_batch *b, double *out) {
  if (!b || !out) return fail("fs_batch_get_boundary_iterate: null argument");
  if (!b->have_state) return fail("fs_batch_get_boundary_iterate: no state yet");
  FS_ON_DEVICE(b);
  // one gather kernel and one transfer through a pinned buffer per call (it is made once per Newton iteration)
  const size_t B = b->d.n_reaches, N = b->d.n_nodes;
  HIP_TRY(b->ends_dev.ensure(4 * B * sizeof(double)));
  HIP_TRY(b->ends_pin.ensure(4 * B * sizeof(double)));
  with_real(b, [&](auto real) {
    using R = decltype(real);
    hipLaunchKernelGGL((gather_boundary_iterate<R>), grid_256(B), dim3(256), 0, b->stream, b->hg.get<const R>(), b->Qg.get<const R>(),
                       b->reach_nodes.get<const int32_t>(), b->ends_dev.get<double>(), B, N);
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(b->ends_pin.get(), b->ends_dev.get(), 4 * B * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  std::memcpy(out, b->ends_pin.get(), 4 * B * sizeof(double));
  return 0;
}

int fs_batch_restart(fs_batch *b, int32_t level, const double *h, const double *Q, const double *h_guess, const double *Q_guess,
                     const double *storage_stage) {
  if (!b || !h || !Q || !h_guess || !Q_guess) return fail("fs_batch_restart: null argument");
  if (level < 0 || level + 1 >= b->d.max_levels) return fail("fs_batch_restart: level out of range");
  if (level > 0 && !storage_stage && b->have_bc[FS_DOWNSTREAM] && b->any_storage[FS_DOWNSTREAM])      // (per-reach kinds: any reach)
    return fail("fs_batch_restart: a storage boundary continues from the reservoir stage of `level` (storage_stage[B], "
                "fs_batch_get_storage_stage); without it the run would go on from stage 0");
  if (fs_batch_set_state(b, h, Q)) return -1;
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches, N = b->d.n_nodes;
  if (upload(b, b->hg, h_guess, B * N) || upload(b, b->Qg, Q_guess, B * N)) return -1;
  if (storage_stage && upload(b, b->Yprev, storage_stage, B)) return -1;
  if (level > 0) {     // the boundary row of `level` (fs_batch_set_state wrote it to row 0) moves to its own row
    HIP_TRY(hipMemcpyAsync(b->hydro.get<char>() + (size_t)level * 4 * B * b->esz, b->hydro.get(), 4 * B * b->esz, hipMemcpyDeviceToDevice, b->stream));
    if (b->hist_h) {
      HIP_TRY(hipMemcpyAsync(b->hist_h.get<char>() + (size_t)level * B * N * b->esz, b->hist_h.get(), B * N * b->esz, hipMemcpyDeviceToDevice, b->stream));
      HIP_TRY(hipMemcpyAsync(b->hist_Q.get<char>() + (size_t)level * B * N * b->esz, b->hist_Q.get(), B * N * b->esz, hipMemcpyDeviceToDevice, b->stream));
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
  }
  b->level = level; b->restart_level = level;
  return 0;
}

int fs_batch_sync(fs_batch *b) {
  if (!b) return fail("null handle");
  FS_ON_DEVICE(b);
  TraceRange range_("flowsim:sync");
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int32_t fs_batch_level(const fs_batch *b) { return b ? b->level : -1; }

int fs_batch_get_state(fs_batch *b, double *h, double *Q) {
  if (!b || !h || !Q) return fail("fs_batch_get_state: null argument");
  FS_ON_DEVICE(b);
  const size_t n = (size_t)b->d.n_reaches * b->d.n_nodes;
  return download(b, h, b->hk, 0, n) || download(b, Q, b->Qk, 0, n) ? -1 : 0;
}

int fs_batch_get_guess(fs_batch *b, double *h, double *Q) {
  if (!b || !h || !Q) return fail("fs_batch_get_guess: null argument");
  FS_ON_DEVICE(b);
  const size_t n = (size_t)b->d.n_reaches * b->d.n_nodes;
  return download(b, h, b->hg, 0, n) || download(b, Q, b->Qg, 0, n) ? -1 : 0;
}

int fs_batch_get_hydrographs(fs_batch *b, int32_t first, int32_t n, double *out) {
  if (!b || !out) return fail("fs_batch_get_hydrographs: null argument");
  FS_ON_DEVICE(b);
  if (check_levels(b, "fs_batch_get_hydrographs", first, n)) return -1;
  const size_t B = b->d.n_reaches;
  return download(b, out, b->hydro, (size_t)first * 4 * B, (size_t)n * 4 * B);
}

int fs_batch_get_iterations(fs_batch *b, int32_t first, int32_t n, int32_t *out) {
  if (!b || !out) return fail("fs_batch_get_iterations: null argument");
  FS_ON_DEVICE(b);
  if (check_levels(b, "fs_batch_get_iterations", first, n)) return -1;
  const size_t B = b->d.n_reaches;
  return fetch(b, out, b->iters.get<int32_t>() + (size_t)first * B, (size_t)n * B * 4);
}

int fs_batch_get_status(fs_batch *b, int32_t *out) {
  if (!b || !out) return fail("fs_batch_get_status: null argument");
  FS_ON_DEVICE(b);
  return fetch(b, out, b->status.get(), (size_t)b->d.n_reaches * 4);
}

int fs_batch_get_history(fs_batch *b, int32_t first, int32_t n, double *h, double *Q) {
  if (!b || !h || !Q) return fail("fs_batch_get_history: null argument");
  FS_ON_DEVICE(b);
  if (!b->hist_h) return fail("fs_batch_get_history: batch was created without FS_FLAG_HISTORY");
  if (check_levels(b, "fs_batch_get_history", first, n)) return -1;
  if (b->restart_level > 0 && first < b->restart_level)
    return fail("fs_batch_get_history: this batch was restarted at level " + std::to_string(b->restart_level) + "; the history before it was not restored");
  const size_t per = (size_t)b->d.n_reaches * b->d.n_nodes;
  return download(b, h, b->hist_h, first * per, n * per) || download(b, Q, b->hist_Q, first * per, n * per) ? -1 : 0;
}

int fs_batch_get_storage_stage(fs_batch *b, double *out) {
  if (!b || !out) return fail("fs_batch_get_storage_stage: null argument");
  FS_ON_DEVICE(b);
  return download(b, out, b->Yprev, 0, b->d.n_reaches);
}

int fs_batch_get_residual_trace(fs_batch *b, int32_t first, int32_t n, double *out) {
  if (!b || !out) return fail("fs_batch_get_residual_trace: null argument");
  FS_ON_DEVICE(b);
  if (!b->trace) return fail("fs_batch_get_residual_trace: batch was created without FS_FLAG_TRACE");
  if (check_levels(b, "fs_batch_get_residual_trace", first, n)) return -1;
  const size_t per = (size_t)FS_TRACE_CAP * b->d.n_reaches;
  return download(b, out, b->trace, first * per, n * per);
}

int fs_batch_get_storage_stages(fs_batch *b, int32_t first, int32_t n, double *out) {
  if (!b || !out) return fail("fs_batch_get_storage_stages: null argument");
  FS_ON_DEVICE(b);
  if (check_levels(b, "fs_batch_get_storage_stages", first, n)) return -1;
  const size_t B = b->d.n_reaches;
  return download(b, out, b->stage_hist, (size_t)first * B, (size_t)n * B);
}

int fs_batch_derive_device(fs_batch *b, int32_t first, int32_t n, int32_t fields) {
  if (!b) return fail("null handle");
  if (!b->hist_h) return fail("fs_batch_derive: batch was created without FS_FLAG_HISTORY");
  if (check_levels(b, "fs_batch_derive", first, n)) return -1;
  if ((fields & FS_DERIVE_ALL) == 0) return fail("fs_batch_derive: no field requested");
  if (b->restart_level > 0 && first < b->restart_level)
    return fail("fs_batch_derive: this batch was restarted at level " + std::to_string(b->restart_level) +
                "; the history before it was not restored (row 0 holds the restart state, which amplitudes then refer to)");
  FS_ON_DEVICE(b);
  TraceRange range_("flowsim:derive");
  const size_t BN = (size_t)b->d.n_reaches * b->d.n_nodes;
  void *dev[8] = {nullptr};
  for (int f = 0; f < 8; ++f) {
    if (!(fields & (1 << f))) continue;
    HIP_TRY(b->derived[f].reserve((f == 7 ? BN : BN * n) * b->esz));
    dev[f] = b->derived[f].get();
  }
  const size_t per_thread = 16 / b->esz;           // one 16-byte access per thread, level and field
  return post_launch(b, "fs_batch_derive", 1, [&](auto real) {      // fs_batch_last_step_ms() then reports this kernel
    using R = decltype(real);
    fs::DeriveArgs<R> a{b->d.n_reaches, b->d.n_nodes, first, n, b->d.section_mode, b->hist_h.get<const R>(), b->hist_Q.get<const R>(),
                        section_tables<R>(b), (R *)dev[0], (R *)dev[1], (R *)dev[2], (R *)dev[3], (R *)dev[4], (R *)dev[5], (R *)dev[6], (R *)dev[7],
                        b->reach_nodes.get<const int32_t>()};
    hipLaunchKernelGGL((fs::derive_fields_kernel<R, (int)(16 / sizeof(R))>), grid_256((BN + per_thread - 1) / per_thread), dim3(256), 0,
                       b->stream, a);
    return true;
  });
}

void *fs_batch_derived_device_ptr(fs_batch *b, int32_t field_index) {
  return (b && field_index >= 0 && field_index < 8) ? b->derived[field_index].get() : nullptr;
}

int fs_batch_derive(fs_batch *b, int32_t first, int32_t n, double *level, double *area, double *top_width,
                    double *froude, double *velocity, double *celerity, double *amplitude, double *peak_amplitude) {
  if (!b) return fail("null handle");
  double *host[8] = {level, area, top_width, froude, velocity, celerity, amplitude, peak_amplitude};
  int fields = 0;
  for (int f = 0; f < 8; ++f) fields |= host[f] ? (1 << f) : 0;
  if (fs_batch_derive_device(b, first, n, fields)) return -1;
  FS_ON_DEVICE(b);
  const size_t BN = (size_t)b->d.n_reaches * b->d.n_nodes;
  for (int f = 0; f < 8; ++f)
    if (host[f] && download(b, host[f], b->derived[f], 0, f == 7 ? BN : BN * n)) return -1;
  return 0;
}

int fs_batch_summarize(fs_batch *b, int32_t first, int32_t n, double *out) {
  if (!b) return fail("fs_batch_summarize: null handle");
  if (!out) return fail("fs_batch_summarize: null output");
  if (check_reduce_range(b, "fs_batch_summarize", first, n)) return -1;
  FS_ON_DEVICE(b);
  TraceRange range_("flowsim:reduce");
  const size_t B = b->d.n_reaches, bytes = (size_t)FS_SUM_NROWS * B * sizeof(double);
  HIP_TRY(b->red_out[0].reserve(bytes));
  if (post_launch(b, "fs_batch_summarize", 0, [&](auto real) {
        return fs::launch_summarize(reduce_args<decltype(real)>(b, first, n), b->red_out[0].get<double>(), b->stream);
      })) return -1;
  return fetch(b, out, b->red_out[0].get(), bytes);
}

// ---- the block a lookup or band call reads: the hydrograph block in the batch's type (fs_batch_lookup, fs_batch_bands), or a block of
// its shape in doubles - the integral block, one gauge's part of the gauge block - on which the shipped kernels run through a
// ReduceArgs<double> that points at it ----
enum class RowSource { kHydrographs, kIntegrals, kGauge };

static const double *source_block(const fs_batch *b, RowSource source, int32_t gauge) {
  if (source == RowSource::kIntegrals) return b->integ.get<const double>();
  return b->gauge.get<const double>() + (size_t)gauge * b->d.max_levels * FS_GAUGE_NROWS * b->d.n_reaches;
}

static fs::ReduceArgs<double> block_args(const fs_batch *b, const double *block, const int32_t *status, int32_t first, int32_t n) {
  return fs::ReduceArgs<double>{block, status, b->iters.get<const int32_t>(), b->d.n_reaches, b->level, first, n};
}

// the handle has gauges and `gauge` is one of them
static int check_gauge(const fs_batch *b, const char *entry, int32_t gauge) {
  if (b->n_gauges == 0 || !b->gauge) return fail(std::string(entry) + ": this batch has no gauges (fs_batch_set_gauges comes first)");
  if (gauge < 0 || gauge >= b->n_gauges)
    return fail(std::string(entry) + ": gauge " + std::to_string(gauge) + " is not one of 0 .. " + std::to_string(b->n_gauges - 1));
  return 0;
}

// fs_batch_lookup and fs_batch_gauge_lookup: lookup_kernel and lookup_finish_kernel over two rows of every level of the range
static int lookup_rows(fs_batch *b, const char *entry, RowSource source, int32_t gauge, int32_t first, int32_t n, int32_t x_row, int32_t y_row,
                       const double *y_offset, const double *xq, int32_t n_q, const double *target, double *values, double *rmse, int32_t *info) {
  if (!b) return fail(std::string(entry) + ": null handle");
  if (!values && !rmse && !info) return fail(std::string(entry) + ": no output requested (values, rmse and info are all NULL)");
  const bool gauges = source == RowSource::kGauge;
  if (gauges ? refuse(fs::check_lookup_args(x_row, y_row, xq, n_q, target, rmse != nullptr, entry, "FS_GAUGE_DEPTH .. FS_GAUGE_VELOCITY"))
             : refuse(fs::check_lookup_args(x_row, y_row, xq, n_q, target, rmse != nullptr))) return -1;
  if (gauges && check_gauge(b, entry, gauge)) return -1;
  if (check_reduce_range(b, entry, first, n)) return -1;
  if (gauges)      // np.interp over rows that hold NaN promises nothing
    for (int32_t k = first; k < first + n; ++k)
      if (!b->gauge_levels[(size_t)k])
        return fail(std::string(entry) + ": level " + std::to_string(k) + " of the range was never evaluated (fs_batch_gauges comes first)");
  FS_ON_DEVICE(b);
  TraceRange range_("flowsim:reduce");
  const size_t B = b->d.n_reaches;
  HIP_TRY(hipStreamSynchronize(b->stream));      // an earlier call's kernels are through with the inputs
  if (y_offset && upload_f64(b->red_in[0], y_offset, B)) return -1;
  if (upload_f64(b->red_in[1], xq, (size_t)n_q)) return -1;
  if (rmse && upload_f64(b->red_in[2], target, (size_t)n_q)) return -1;
  const fs::LookupLayout lay = fs::lookup_layout((size_t)n_q, B);
  HIP_TRY(b->red_out[1].reserve(lay.bytes));
  double *blk = b->red_out[1].get<double>();
  fs::LookupArgs l;
  l.x_row = x_row; l.y_row = y_row; l.n_q = n_q;
  l.y_offset = y_offset ? b->red_in[0].get<const double>() : nullptr;
  l.xq = b->red_in[1].get<const double>(); l.target = rmse ? b->red_in[2].get<const double>() : nullptr;
  l.values = blk + lay.values; l.rmse = rmse ? blk + lay.rmse : nullptr; l.info = info ? (int32_t *)(blk + lay.info) : nullptr;
  if (post_launch(b, entry, 0, [&](auto real) {
        if (!gauges) return fs::launch_lookup(reduce_args<decltype(real)>(b, first, n), l, b->stream);
        return fs::launch_lookup(block_args(b, source_block(b, source, gauge), b->status.get<const int32_t>(), first, n), l, b->stream);
      })) return -1;
  if (values && fetch(b, values, l.values, lay.n_values * sizeof(double))) return -1;
  if (rmse && fetch(b, rmse, l.rmse, B * sizeof(double))) return -1;
  if (info && fetch(b, info, l.info, B * sizeof(int32_t))) return -1;
  return 0;
}

int fs_batch_lookup(fs_batch *b, int32_t first, int32_t n, int32_t x_row, int32_t y_row, const double *y_offset,
                    const double *xq, int32_t n_q, const double *target, double *values, double *rmse, int32_t *info) {
  return lookup_rows(b, "fs_batch_lookup", RowSource::kHydrographs, -1, first, n, x_row, y_row, y_offset, xq, n_q, target, values, rmse, info);
}

int fs_batch_gauge_lookup(fs_batch *b, int32_t gauge, int32_t first, int32_t n, int32_t x_row, int32_t y_row, const double *y_offset,
                          const double *xq, int32_t n_q, const double *target, double *values, double *rmse, int32_t *info) {
  return lookup_rows(b, "fs_batch_gauge_lookup", RowSource::kGauge, gauge, first, n, x_row, y_row, y_offset, xq, n_q, target, values, rmse, info);
}

int fs_batch_envelope_device(fs_batch *b, int32_t first, int32_t n, int32_t quantities, const double *threshold,
                             int32_t threshold_per_reach, int32_t threshold_quantity) {
  if (!b) return fail("fs_batch_envelope: null handle");
  if (!b->hist_h) return fail("fs_batch_envelope: batch was created without FS_FLAG_HISTORY");
  if ((quantities & FS_ENV_ALL) == 0 || (quantities & ~FS_ENV_ALL) != 0)
    return fail("fs_batch_envelope: quantities must be a mask of FS_ENV_DEPTH .. FS_ENV_TOP_WIDTH with at least one bit set");
  const int cross_q = threshold ? fs::EnvRows::quantity_index(threshold_quantity) : -1;
  if (threshold && cross_q < 0) return fail("fs_batch_envelope: threshold_quantity must be one of FS_ENV_DEPTH .. FS_ENV_TOP_WIDTH");
  if (check_reduce_range(b, "fs_batch_envelope", first, n, "the history before it was not restored")) return -1;
  FS_ON_DEVICE(b);
  TraceRange range_("flowsim:envelope");
  const size_t B = b->d.n_reaches, BN = B * b->d.n_nodes;
  const fs::EnvRows rows(quantities, threshold != nullptr);
  b->env_quantities = 0; b->env_crossings = false;      // (the handle holds no envelope until this one is launched)
  HIP_TRY(hipStreamSynchronize(b->stream));             // an earlier call's kernels are through with the threshold
  if (threshold && upload(b, b->env_thr, threshold, threshold_per_reach ? BN : (size_t)b->d.n_nodes)) return -1;
  HIP_TRY(b->env_out.reserve((size_t)rows.n_rows * BN * sizeof(double)));
  HIP_TRY(b->env_levels.reserve(B * sizeof(int32_t)));
  const char *unroll_env = std::getenv("FS_ENVELOPE_UNROLL");      // levels whose loads a thread has in flight: 1, 4, 8 (tools/time_envelope.py compares)
  const int unroll = unroll_env ? std::atoi(unroll_env) : 0;       // 0: the launcher's choice
  if (post_launch(b, "fs_batch_envelope", 1, [&](auto real) {      // fs_batch_last_step_ms() then reports this kernel
        using R = decltype(real);
        fs::EnvelopeArgs<R> a{b->d.n_reaches, b->d.n_nodes, first, n, b->d.section_mode, b->hist_h.get<const R>(), b->hist_Q.get<const R>(),
                              section_tables<R>(b), b->reach_nodes.get<const int32_t>(), reduce_args<R>(b, first, n), quantities, cross_q,
                              threshold ? b->env_thr.get<const R>() : nullptr, threshold_per_reach ? 1 : 0, b->env_out.get<double>(),
                              threshold ? b->env_out.get<double>() + (size_t)rows.cross_row * BN : nullptr, b->env_levels.get<int32_t>()};
        return fs::launch_envelope(a, unroll, b->stream);
      })) return -1;
  b->env_quantities = quantities; b->env_crossings = threshold != nullptr;
  return 0;
}

void *fs_batch_envelope_device_ptr(fs_batch *b, int32_t row) {
  if (!b) { fail("fs_batch_envelope_device_ptr: null handle"); return nullptr; }
  const int n_rows = fs::EnvRows(b->env_quantities, b->env_crossings).n_rows;
  if (row < 0 || row >= n_rows) { fail("fs_batch_envelope_device_ptr: the envelope this handle holds has no such row"); return nullptr; }
  return b->env_out.get<double>() + (size_t)row * b->d.n_reaches * b->d.n_nodes;
}

int fs_batch_envelope(fs_batch *b, int32_t first, int32_t n, int32_t quantities, const double *threshold, int32_t threshold_per_reach,
                      int32_t threshold_quantity, double *out, double *crossing, int32_t *levels) {
  if (!b) return fail("fs_batch_envelope: null handle");
  if (crossing && !threshold) return fail("fs_batch_envelope: crossings need a threshold");
  if (fs_batch_envelope_device(b, first, n, quantities, threshold, threshold_per_reach, threshold_quantity)) return -1;
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches, BN = B * b->d.n_nodes;
  const size_t n_out = (size_t)fs::EnvRows(quantities, threshold != nullptr).cross_row * BN;
  if (out && fetch(b, out, b->env_out.get(), n_out * sizeof(double))) return -1;
  if (crossing && fetch(b, crossing, b->env_out.get<double>() + n_out, (size_t)FS_ENV_NCROSS * BN * sizeof(double))) return -1;
  if (levels && fetch(b, levels, b->env_levels.get(), B * sizeof(int32_t))) return -1;
  return 0;
}

int fs_batch_profile_bands(fs_batch *b, int32_t quantity, int32_t stat, const double *q, int32_t n_q, double *moments, double *quantiles,
                           double *exceed, int32_t *n_members) {
  if (!b) return fail("fs_batch_profile_bands: null handle");
  if (!moments && !quantiles && !exceed && !n_members)
    return fail("fs_batch_profile_bands: no output requested (moments, quantiles, exceed and n_members are all NULL)");
  if (refuse(fs::check_quantile_levels("fs_batch_profile_bands", q, n_q))) return -1;
  if (b->env_quantities == 0) return fail("fs_batch_profile_bands: this handle holds no envelope (fs_batch_envelope comes first)");
  const fs::EnvRows held(b->env_quantities, b->env_crossings);
  const int row = held.row_of(quantity, stat);
  if (row < 0) return fail("fs_batch_profile_bands: the envelope this handle holds has no such row (quantity " + std::to_string(quantity) +
                           ", statistic " + std::to_string(stat) + ")");
  if (exceed && !b->env_crossings) return fail("fs_batch_profile_bands: exceed needs an envelope that was computed with a threshold");
  FS_ON_DEVICE(b);
  TraceRange range_("flowsim:reduce");
  const int B = b->d.n_reaches, N = b->d.n_nodes;
  const size_t BN = (size_t)B * N;
  const bool want_q = quantiles && n_q > 0;
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (want_q && upload_f64(b->red_in[1], q, (size_t)n_q)) return -1;
  HIP_TRY(b->env_t.reserve((exceed ? 2 : 1) * BN * sizeof(double)));
  const fs::BandLayout lay = fs::band_layout((size_t)N, 1, want_q ? (size_t)n_q : 0, true);      // (the exceed row is always reserved)
  HIP_TRY(b->red_out[2].reserve(lay.bytes));
  double *blk = b->red_out[2].get<double>();
  const double *env = b->env_out.get<const double>();
  fs::TransposeRows rows{{env + (size_t)row * BN, env + (size_t)(held.cross_row + FS_ENV_CROSS_COUNT) * BN}};
  fs::ProfileBandArgs p;
  p.x = b->env_t.get<const double>(); p.count = exceed ? p.x + BN : nullptr;
  p.status = b->status.get<const int32_t>(); p.levels = b->env_levels.get<const int32_t>(); p.reach_nodes = b->reach_nodes.get<const int32_t>();
  p.B = B; p.N = N;
  point_bands(p, lay, blk, b->red_in[1].get<const double>(), n_q, moments != nullptr, n_members != nullptr);
  p.exceed = exceed ? blk + lay.extra : nullptr;
  if (post_launch(b, "fs_batch_profile_bands", 2, [&](auto) {      // fs_batch_last_step_ms(): the transpose and the bands
        return fs::launch_transpose_rows(rows, exceed ? 2 : 1, b->env_t.get<double>(), B, N, b->stream) && fs::launch_profile_bands(p, b->stream);
      })) return -1;
  return fetch_bands(b, lay, blk, moments, quantiles, exceed, n_members);
}

// ---- reach integrals and the water balance (fs_balance.hpp) ----

// the handle's integral block and its marks exist (first use: every row NaN), and the fp64 scheme of every reach is on the device
static int ready_integrals(fs_batch *b, const char *entry) {
  const size_t B = b->d.n_reaches, L = b->d.max_levels;
  if (!b->integ) {
    HIP_TRY(b->integ.ensure(L * FS_INT_NROWS * B * sizeof(double)));
    HIP_TRY(b->integ_mark.ensure(L * B * sizeof(int32_t)));
    if (!fs::launch_clear_integrals(b->integ.get<double>(), L * FS_INT_NROWS * B, b->integ_mark.get<int32_t>(), L * B, b->stream)) {
      b->integ.reset(); b->integ_mark.reset();
      return fail(std::string(entry) + kNoReduceKernels);
    }
    HIP_TRY(hipGetLastError());
  }
  if (b->bal_scheme_stale || !b->bal_scheme) {
    const double wide[3] = {b->theta, b->dt, b->dx};
    const std::vector<double> v = fs::reach_scheme_rows(b->rs_host, wide, 3, B, true);
    HIP_TRY(hipStreamSynchronize(b->stream));      // an earlier call's kernels are through with the values before
    if (upload_f64(b->bal_scheme, v.data(), v.size())) return -1;
    b->bal_scheme_stale = false;
  }
  return 0;
}

int fs_batch_reach_integrals(fs_batch *b, int32_t first, int32_t n, const double *threshold, int32_t threshold_per_reach) {
  if (!b) return fail("fs_batch_reach_integrals: null handle");
  if (!b->have_scheme || !b->have_geo) return fail("fs_batch_reach_integrals: the scheme (fs_batch_set_scheme: dx) and the geometry must be set first");
  const bool current = first == -1;
  if (current) {
    if (n != 1) return fail("fs_batch_reach_integrals: first = -1 evaluates the current state, one row: n must be 1");
    if (!b->have_state) return fail("fs_batch_reach_integrals: no state yet");
    if (b->iterating) return fail("fs_batch_reach_integrals: a level opened with fs_batch_iterate must be closed first");
  } else {
    if (!b->hist_h) return fail("fs_batch_reach_integrals: batch was created without FS_FLAG_HISTORY (first = -1 evaluates the current state)");
    if (check_reduce_range(b, "fs_batch_reach_integrals", first, n)) return -1;
  }
  FS_ON_DEVICE(b);
  TraceRange range_("flowsim:balance");
  const size_t B = b->d.n_reaches, BN = B * b->d.n_nodes;
  if (ready_integrals(b, "fs_batch_reach_integrals")) return -1;
  if (threshold) {
    HIP_TRY(hipStreamSynchronize(b->stream));             // an earlier call's kernels are through with the threshold
    if (upload(b, b->integ_thr, threshold, threshold_per_reach ? BN : (size_t)b->d.n_nodes)) return -1;
  }
  const int32_t row0 = current ? b->level : first;
  return post_launch(b, "fs_batch_reach_integrals", 1, [&](auto real) {      // fs_batch_last_step_ms() then reports this kernel
    using R = decltype(real);
    fs::IntegralArgs<R> a{b->d.n_reaches, b->d.n_nodes, b->d.section_mode,
                          current ? b->hk.get<const R>() : b->hist_h.get<const R>() + (size_t)first * BN, current ? (int64_t)0 : (int64_t)BN,
                          section_tables<R>(b), b->reach_nodes.get<const int32_t>(), reduce_args<R>(b, row0, n),
                          b->bal_scheme.get<const double>() + 2 * B, threshold ? b->integ_thr.get<const R>() : nullptr,
                          threshold_per_reach ? 1 : 0, b->integ.get<double>(), b->integ_mark.get<int32_t>()};
    return fs::launch_reach_integrals(a, b->stream);
  });
}

int fs_batch_water_balance(fs_batch *b, int32_t first, int32_t n, double *totals) {
  if (!b) return fail("fs_batch_water_balance: null handle");
  if (!b->have_scheme) return fail("fs_batch_water_balance: the scheme (fs_batch_set_scheme: theta, dt) must be set first");
  if (check_reduce_range(b, "fs_batch_water_balance", first, n)) return -1;
  FS_ON_DEVICE(b);
  TraceRange range_("flowsim:balance");
  const size_t B = b->d.n_reaches, bytes = (size_t)FS_BAL_NROWS * B * sizeof(double);
  if (ready_integrals(b, "fs_batch_water_balance")) return -1;
  if (totals) HIP_TRY(b->red_out[0].reserve(bytes));
  fs::BalanceArgs p{b->integ.get<double>(), b->integ_mark.get<const int32_t>(), b->bal_scheme.get<const double>(),
                    b->bal_scheme.get<const double>() + B, totals ? b->red_out[0].get<double>() : nullptr};
  if (post_launch(b, "fs_batch_water_balance", 1, [&](auto real) { return fs::launch_balance(reduce_args<decltype(real)>(b, first, n), p, b->stream); }))
    return -1;
  return totals ? fetch(b, totals, p.totals, bytes) : 0;
}

int fs_batch_get_reach_integrals(fs_batch *b, int32_t first, int32_t n, double *out) {
  if (!b || !out) return fail("fs_batch_get_reach_integrals: null argument");
  if (check_levels(b, "fs_batch_get_reach_integrals", first, n)) return -1;
  FS_ON_DEVICE(b);
  if (ready_integrals(b, "fs_batch_get_reach_integrals")) return -1;
  const size_t B = b->d.n_reaches;
  return fetch(b, out, b->integ.get<double>() + (size_t)first * FS_INT_NROWS * B, (size_t)n * FS_INT_NROWS * B * sizeof(double));
}

void *fs_batch_reach_integrals_device_ptr(fs_batch *b) { return b ? b->integ.get() : nullptr; }

// fs_batch_bands, fs_batch_integral_bands and fs_batch_gauge_bands: bands_kernel over the four rows of every level of the range - of the
// hydrograph block, or (the call is then timed) of the integral block or of one gauge's block, which have its shape.  A gauge's bands
// leave out, with the failed members, those that do not have the gauge: gauge_members_kernel writes the status bands_kernel reads.
static int band_rows(fs_batch *b, const char *entry, RowSource source, int32_t gauge, int32_t first, int32_t n, const double *q, int32_t n_q,
                     double *moments, double *quantiles, int32_t *n_members) {
  if (!b) return fail(std::string(entry) + ": null handle");
  if (!moments && !quantiles && !n_members) return fail(std::string(entry) + ": no output requested (moments, quantiles and n_members are all NULL)");
  if (source == RowSource::kGauge && check_gauge(b, entry, gauge)) return -1;
  if (refuse(fs::check_quantile_levels(entry, q, n_q)) || check_reduce_range(b, entry, first, n)) return -1;
  FS_ON_DEVICE(b);
  TraceRange range_("flowsim:reduce");
  if (source == RowSource::kIntegrals && ready_integrals(b, entry)) return -1;
  if (source == RowSource::kGauge) HIP_TRY(b->gauge_members.ensure((size_t)b->d.n_reaches * sizeof(int32_t)));
  const bool want_q = quantiles && n_q > 0;
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (want_q && upload_f64(b->red_in[1], q, (size_t)n_q)) return -1;
  static_assert(FS_INT_NROWS == 4 && FS_GAUGE_NROWS == 4, "bands_kernel walks the four rows of a level of the hydrograph block");
  const fs::BandLayout lay = fs::band_layout((size_t)n, 4, want_q ? (size_t)n_q : 0, false);
  HIP_TRY(b->red_out[2].reserve(lay.bytes));
  double *blk = b->red_out[2].get<double>();
  fs::BandArgs p;
  point_bands(p, lay, blk, b->red_in[1].get<const double>(), n_q, moments != nullptr, n_members != nullptr);
  const int launches = source == RowSource::kHydrographs ? 0 : source == RowSource::kIntegrals ? 1 : 2;
  if (post_launch(b, entry, launches, [&](auto real) {
        if (source == RowSource::kHydrographs) return fs::launch_bands(reduce_args<decltype(real)>(b, first, n), p, b->stream);
        const int32_t *status = b->status.get<const int32_t>();
        if (source == RowSource::kGauge) {
          if (!fs::launch_gauge_members(status, b->reach_nodes.get<const int32_t>(), b->gauge_node.get<const int32_t>(),
                                        b->gauge_weight.get<const double>(), b->n_gauges, gauge, b->gauge_per_reach ? 1 : 0, b->d.n_nodes,
                                        b->d.n_reaches, b->gauge_members.get<int32_t>(), b->stream)) return false;
          status = b->gauge_members.get<const int32_t>();
        }
        return fs::launch_bands(block_args(b, source_block(b, source, gauge), status, first, n), p, b->stream);
      })) return -1;
  return fetch_bands(b, lay, blk, moments, quantiles, nullptr, n_members);
}

int fs_batch_bands(fs_batch *b, int32_t first, int32_t n, const double *q, int32_t n_q, double *moments, double *quantiles,
                   int32_t *n_members) {
  return band_rows(b, "fs_batch_bands", RowSource::kHydrographs, -1, first, n, q, n_q, moments, quantiles, n_members);
}

int fs_batch_integral_bands(fs_batch *b, int32_t first, int32_t n, const double *q, int32_t n_q, double *moments, double *quantiles,
                            int32_t *n_members) {
  return band_rows(b, "fs_batch_integral_bands", RowSource::kIntegrals, -1, first, n, q, n_q, moments, quantiles, n_members);
}

int fs_batch_gauge_bands(fs_batch *b, int32_t gauge, int32_t first, int32_t n, const double *q, int32_t n_q, double *moments,
                         double *quantiles, int32_t *n_members) {
  return band_rows(b, "fs_batch_gauge_bands", RowSource::kGauge, gauge, first, n, q, n_q, moments, quantiles, n_members);
}

// ---- interior gauges (fs_gauge.hpp) ----

int fs_batch_set_gauges(fs_batch *b, int32_t n_gauges, const int32_t *node, const double *weight, int32_t per_reach) {
  if (!b) return fail("fs_batch_set_gauges: null handle");
  const size_t B = b->d.n_reaches, L = b->d.max_levels;
  const size_t count = n_gauges > 0 ? (size_t)n_gauges * (per_reach ? B : 1) : 0;
  if (refuse(fs::check_gauge_list("fs_batch_set_gauges", n_gauges, node, weight, count, b->d.n_nodes))) return -1;
  FS_ON_DEVICE(b);
  HIP_TRY(hipStreamSynchronize(b->stream));      // an earlier call's kernels are through with the positions and the block
  b->n_gauges = 0; b->gauge_per_reach = false; b->gauge_levels.clear();
  if (n_gauges == 0) {
    for (fs::DeviceBuffer *p : {&b->gauge, &b->gauge_mark, &b->gauge_node, &b->gauge_weight, &b->gauge_members}) p->reset();
    return 0;
  }
  const fs::GaugeLayout lay{(size_t)n_gauges, L, B};
  struct Want { fs::DeviceBuffer *buf; size_t bytes; const char *what; };
  const Want wants[] = {{&b->gauge, lay.block() * sizeof(double), "the gauge block [n_gauges][max_levels][4][B] of doubles"},
                        {&b->gauge_mark, lay.marks() * sizeof(int32_t), "the gauge marks [max_levels][B] of int32"}};
  for (const Want &w : wants) {
    const hipError_t e = w.buf->ensure(w.bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      b->gauge.reset(); b->gauge_mark.reset();
      return fail(std::string("fs_batch_set_gauges: cannot allocate ") + w.what + ", " + std::to_string(w.bytes) + " bytes: " + hipGetErrorString(e));
    }
  }
  HIP_TRY(b->gauge_node.ensure(count * sizeof(int32_t)));
  HIP_TRY(b->gauge_weight.ensure(count * sizeof(double)));
  HIP_TRY(hipMemcpy(b->gauge_node.get(), node, count * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->gauge_weight.get(), weight, count * sizeof(double), hipMemcpyHostToDevice));
  if (!fs::launch_clear_integrals(b->gauge.get<double>(), lay.block(), b->gauge_mark.get<int32_t>(), lay.marks(), b->stream)) {
    b->gauge.reset(); b->gauge_mark.reset();
    return fail(std::string("fs_batch_set_gauges") + kNoReduceKernels);
  }
  HIP_TRY(hipGetLastError());
  b->n_gauges = n_gauges; b->gauge_per_reach = per_reach != 0;
  b->gauge_levels.assign(L, 0);
  return 0;
}

int fs_batch_gauges(fs_batch *b, int32_t first, int32_t n) {
  if (!b) return fail("fs_batch_gauges: null handle");
  if (check_gauge(b, "fs_batch_gauges", 0)) return -1;
  if (!b->have_geo) return fail("fs_batch_gauges: the geometry must be set first");
  const bool current = first == -1;
  if (current) {
    if (n != 1) return fail("fs_batch_gauges: first = -1 evaluates the current state, one row: n must be 1");
    if (!b->have_state) return fail("fs_batch_gauges: no state yet");
    if (b->iterating) return fail("fs_batch_gauges: a level opened with fs_batch_iterate must be closed first");
  } else {
    if (!b->hist_h) return fail("fs_batch_gauges: batch was created without FS_FLAG_HISTORY (first = -1 evaluates the current state)");
    if (check_reduce_range(b, "fs_batch_gauges", first, n, "the history before it was not restored")) return -1;
  }
  FS_ON_DEVICE(b);
  TraceRange range_("flowsim:gauges");
  const size_t BN = (size_t)b->d.n_reaches * b->d.n_nodes;
  const int32_t row0 = current ? b->level : first;
  if (post_launch(b, "fs_batch_gauges", 1, [&](auto real) {      // fs_batch_last_step_ms() then reports this kernel
        using R = decltype(real);
        fs::GaugeArgs<R> a{b->d.n_reaches, b->d.n_nodes, b->d.section_mode, b->n_gauges,
                           current ? b->hk.get<const R>() : b->hist_h.get<const R>() + (size_t)first * BN,
                           current ? b->Qk.get<const R>() : b->hist_Q.get<const R>() + (size_t)first * BN, current ? (int64_t)0 : (int64_t)BN,
                           section_tables<R>(b), b->reach_nodes.get<const int32_t>(), reduce_args<R>(b, row0, n),
                           b->gauge_node.get<const int32_t>(), b->gauge_weight.get<const double>(), b->gauge.get<double>(),
                           b->gauge_mark.get<int32_t>(), b->d.max_levels};
        return fs::launch_gauge_gather(a, b->gauge_per_reach, b->stream);
      })) return -1;
  std::fill(b->gauge_levels.begin() + row0, b->gauge_levels.begin() + row0 + n, 1);
  return 0;
}

int fs_batch_get_gauges(fs_batch *b, int32_t gauge, int32_t first, int32_t n, double *out) {
  if (!b || !out) return fail("fs_batch_get_gauges: null argument");
  if (check_gauge(b, "fs_batch_get_gauges", gauge) || check_levels(b, "fs_batch_get_gauges", first, n)) return -1;
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches;
  return fetch(b, out, source_block(b, RowSource::kGauge, gauge) + (size_t)first * FS_GAUGE_NROWS * B, (size_t)n * FS_GAUGE_NROWS * B * sizeof(double));
}

void *fs_batch_gauges_device_ptr(fs_batch *b, int32_t gauge) {
  if (!b || !b->gauge || gauge < 0 || gauge >= b->n_gauges) return nullptr;
  return const_cast<double *>(source_block(b, RowSource::kGauge, gauge));
}

int fs_batch_gauge_score(fs_batch *b, int32_t gauge, int32_t signal, int32_t first, int32_t n, const double *observed,
                         int32_t observed_per_reach, double *out) {
  if (!b) return fail("fs_batch_gauge_score: null handle");
  if (!observed || !out) return fail("fs_batch_gauge_score: null observations or output");
  if (check_gauge(b, "fs_batch_gauge_score", gauge)) return -1;
  if (signal < 0 || signal >= FS_GAUGE_NROWS)
    return fail("fs_batch_gauge_score: signal " + std::to_string(signal) + " is not one of FS_GAUGE_DEPTH .. FS_GAUGE_VELOCITY (0 .. 3)");
  if (check_reduce_range(b, "fs_batch_gauge_score", first, n)) return -1;
  FS_ON_DEVICE(b);
  TraceRange range_("flowsim:gauges");
  const size_t B = b->d.n_reaches, bytes = (size_t)FS_GS_NROWS * B * sizeof(double);
  HIP_TRY(hipStreamSynchronize(b->stream));      // an earlier call's kernels are through with the observations
  if (upload_f64(b->red_in[0], observed, (size_t)n * (observed_per_reach ? B : 1))) return -1;
  HIP_TRY(b->red_out[0].reserve(bytes));
  const fs::ScoreArgs p{source_block(b, RowSource::kGauge, gauge), b->gauge_mark.get<const int32_t>(), gauge, signal, b->red_in[0].get<const double>(),
                        observed_per_reach ? 1 : 0, b->red_out[0].get<double>()};
  if (post_launch(b, "fs_batch_gauge_score", 1, [&](auto) {
        return fs::launch_gauge_score(block_args(b, p.gauge, b->status.get<const int32_t>(), first, n), p, b->stream);
      })) return -1;
  return fetch(b, out, p.out, bytes);
}

// ---- assimilation of gauge observations (fs_assim.hpp) ----

int fs_batch_assimilate(fs_batch *b, int32_t n_obs, const int32_t *gauge, const int32_t *signal, const double *value,
                        const double *variance, const double *perturb, const double *taper, double depth_floor, double *prior,
                        double *cross_cov, int32_t *clamped, int32_t *n_active) {
  const char *entry = "fs_batch_assimilate";
  if (!b) return fail("fs_batch_assimilate: null handle");
  if (!b->have_state) return fail("fs_batch_assimilate: no state yet");
  if (!b->have_geo) return fail("fs_batch_assimilate: the geometry must be set first");
  if (check_gauge(b, entry, 0)) return -1;
  if (b->gauge_per_reach) return fail("fs_batch_assimilate: the gauges were set per reach; the members of an analysis share their positions");
  if (b->reach_nodes) return fail("fs_batch_assimilate: per-reach node counts were given; the members of an analysis are one channel, node for node");
  if (b->iterating) return fail("fs_batch_assimilate: a level opened with fs_batch_iterate must be closed first");
  const size_t B = b->d.n_reaches, N = b->d.n_nodes, L = b->d.max_levels;
  if (refuse(fs::check_observations(entry, n_obs, gauge, signal, value, variance, perturb, taper, depth_floor, b->n_gauges, B, N))) return -1;
  if (fs_batch_gauges(b, -1, 1)) return -1;                   // the row of the current level, from the current state
  FS_ON_DEVICE(b);
  TraceRange range_("flowsim:assimilate");
  const size_t m = (size_t)n_obs, level = (size_t)b->level;
  std::vector<int32_t> mark(B), active(B);
  std::vector<double> y(m * B);
  if (fetch(b, mark.data(), b->gauge_mark.get<const int32_t>() + level * B, B * sizeof(int32_t))) return -1;
  for (size_t j = 0; j < m; ++j)
    if (fetch(b, y.data() + j * B, b->gauge.get<const double>() + (((size_t)gauge[j] * L + level) * FS_GAUGE_NROWS + (size_t)signal[j]) * B,
              B * sizeof(double))) return -1;
  uint32_t need = 0;
  for (size_t j = 0; j < m; ++j) need |= 1u << gauge[j];
  int32_t first_active = -1;
  for (size_t r = 0; r < B; ++r) {
    active[r] = ((uint32_t)mark[r] & need) == need;
    if (active[r] && first_active < 0) first_active = (int32_t)r;
  }
  std::vector<double> ybar, S, Cov, Lc, Z;
  int32_t na = 0;
  const std::string text = fs::analysis_coefficients(entry, n_obs, B, active.data(), [&](size_t j, size_t r) { return y[j * B + r]; }, value,
                                                     variance, perturb, ybar, S, Cov, Lc, Z, &na);
  if (n_active) *n_active = na;
  if (refuse(text)) return -1;
  // S and Z member-major, padded with zero rows to the bucket the kernels are instantiated on
  const fs::AssimLayout lay{B, N, m};
  std::vector<double> cols(2 * lay.columns(), 0.0);
  for (size_t r = 0; r < B; ++r)
    for (size_t j = 0; j < m; ++j) {
      cols[lay.column(r) + j] = S[j * B + r];
      cols[lay.columns() + lay.column(r) + j] = Z[j * B + r];
    }
  std::vector<int32_t> flags(2 * B, 0);
  std::copy(active.begin(), active.end(), flags.begin());
  HIP_TRY(b->assim_part.reserve(lay.partials() * sizeof(double)));
  HIP_TRY(b->assim_out.reserve((lay.prior() + lay.cross()) * sizeof(double)));
  if (upload_f64(b->assim_cols, cols.data(), cols.size())) return -1;
  if (taper && upload_f64(b->assim_taper, taper, m * N)) return -1;
  HIP_TRY(b->assim_flags.reserve(flags.size() * sizeof(int32_t)));
  HIP_TRY(hipMemcpy(b->assim_flags.get(), flags.data(), flags.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  if (post_launch(b, entry, 3, [&](auto real) {             // fs_batch_last_step_ms() then reports the moments, combine and update kernels
        using R = decltype(real);
        const fs::AssimArgs<R> a{(int32_t)B, (int32_t)N, n_obs, na, first_active, b->hk.get<R>(), b->Qk.get<R>(), b->hg.get<R>(), b->Qg.get<R>(),
                                 b->assim_flags.get<const int32_t>(), b->assim_cols.get<const double>(),
                                 b->assim_cols.get<const double>() + lay.columns(), taper ? b->assim_taper.get<const double>() : nullptr,
                                 depth_floor, b->assim_part.get<double>(), b->assim_out.get<double>(), b->assim_out.get<double>() + lay.prior(),
                                 b->assim_flags.get<int32_t>() + B};
        return fs::launch_assimilate(a, b->stream);
      })) return -1;
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (prior && fetch(b, prior, b->assim_out.get<const double>(), lay.prior() * sizeof(double))) return -1;
  if (cross_cov && fetch(b, cross_cov, b->assim_out.get<const double>() + lay.prior(), lay.cross() * sizeof(double))) return -1;
  if (clamped && fetch(b, clamped, b->assim_flags.get<const int32_t>() + B, B * sizeof(int32_t))) return -1;
  return 0;
}

void *fs_batch_hydrograph_device_ptr(fs_batch *b) { return b ? b->hydro.get() : nullptr; }
void *fs_batch_stream(fs_batch *b) { return b ? (void *)b->stream : nullptr; }

double fs_batch_last_step_ms(fs_batch *b) {
  if (!b || !b->timed) return -1.0;
  float ms = 0.f;
  if (hipEventSynchronize(b->ev1) != hipSuccess) return -1.0;
  if (hipEventElapsedTime(&ms, b->ev0, b->ev1) != hipSuccess) return -1.0;
  return (double)ms;
}

int32_t fs_batch_last_launch_count(fs_batch *b) { return b ? b->launches : 0; }

#ifdef FS_STAMP
// diagnostic builds only: out[B][16][12] cycle sums (waves beyond W are zero)
int fs_debug_stamps(fs_batch *b, unsigned long long *out) {
  if (!b || !out || !b->dbg) return fail("fs_debug_stamps: not available");
  return fetch(b, out, b->dbg.get(), (size_t)b->d.n_reaches * 16 * 12 * 8);
}
#endif

int32_t fs_kernel_table_size(void) { return kNumEntries; }

int fs_kernel_table_entry(int32_t i, int32_t *out) {
  if (i < 0 || i >= kNumEntries || !out) return fail("fs_kernel_table_entry: index out of range");
  const fs::KernelKey &e = kEntries[i].key;
  out[0] = e.dtype; out[1] = e.sec; out[2] = e.M; out[3] = e.W; out[4] = e.full; out[5] = e.bck; out[6] = e.diag; out[7] = e.longk;
  return 0;
}

int32_t fs_batch_kernel_index(fs_batch *b) { return (b && b->kern) ? (int32_t)(b->kern - kEntries) : -1; }

int32_t fs_kernel_table_entry_tail(int32_t i) { return (i >= 0 && i < kNumEntries) ? kEntries[i].key.tail : -2; }
int32_t fs_kernel_table_entry_team(int32_t i) { return (i >= 0 && i < kNumEntries) ? kEntries[i].key.team : -2; }

int32_t fs_batch_poly_tables(fs_batch *b) { return (b && b->poly_x) ? (b->poly_K > 0 ? 1 : 0) : -1; }

int fs_batch_get_stage_table(fs_batch *b, int32_t reach, int32_t node, double *out) {
  if (!b || !out) return fail("fs_batch_get_stage_table: null argument");
  if (!b->poly_x) return fail("fs_batch_get_stage_table: no polylines set");
  if (b->poly_K <= 0) return fail("fs_batch_get_stage_table: this batch walks its polylines' edges and holds no stage tables (fs_batch_poly_tables)");
  if (reach < 0 || reach >= b->d.n_reaches || node < 0 || node >= b->d.n_nodes) return fail("fs_batch_get_stage_table: reach or node out of range");
  FS_ON_DEVICE(b);
  const size_t N = b->d.n_nodes, P = b->poly_K, KP = fs::poly_table_bp((int)P), i = node;
  const double *tz = b->poly_tz.get<const double>() + (b->poly_reach_stride ? (size_t)reach * N * fs::poly_table_stride((int)P) : 0);
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(out, tz + i * KP, KP * sizeof(double), hipMemcpyDeviceToHost));
  // the node's 16-byte pairs, N pairs apart in the node-minor layout, in build_stage_table's order
  HIP_TRY(hipMemcpy2D(out + KP, 2 * sizeof(double), tz + N * KP + 2 * i, N * 2 * sizeof(double), 2 * sizeof(double), P * (fs::FS_PT_BLOCK / 2),
                      hipMemcpyDeviceToHost));
  return 0;
}

int fs_batch_get_bed_levels(fs_batch *b, double *out) {
  if (!b || !out) return fail("fs_batch_get_bed_levels: null argument");
  if (!b->geo_table) return fail("fs_batch_get_bed_levels: no TABLE or IRREGULAR geometry set");
  FS_ON_DEVICE(b);
  const size_t B = b->d.n_reaches, N = b->d.n_nodes, rows = b->geo_reach_stride ? B : 1, esz = b->esz;
  // row Z_BED of every table (one shared by the batch, or one per reach, geo_reach_stride elements apart) in the batch's type
  std::vector<char> raw(rows * N * esz);
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy2D(raw.data(), N * esz, b->geo_table.get<const char>() + (size_t)FS_GEO_Z_BED * N * esz, (rows > 1 ? b->geo_reach_stride : N) * esz, N * esz, rows,
                      hipMemcpyDeviceToHost));
  for (size_t r = 0; r < B; ++r)
    for (size_t i = 0; i < N; ++i) {
      const size_t q = (rows > 1 ? r : 0) * N + i;
      out[r * N + i] = esz == sizeof(double) ? reinterpret_cast<const double *>(raw.data())[q] : (double)reinterpret_cast<const float *>(raw.data())[q];
    }
  return 0;
}

int fs_batch_kernel_info(fs_batch *b, int32_t *cells_per_thread, int32_t *waves_per_reach, int32_t *lds_bytes,
                         int32_t *vgprs) {
  if (!b) return fail("null handle");
  hipFuncAttributes at;
  HIP_TRY(hipFuncGetAttributes(&at, b->kern->kp));
  if (cells_per_thread) *cells_per_thread = b->kern->key.M;
  if (waves_per_reach) *waves_per_reach = b->kern->key.W;
  if (lds_bytes) *lds_bytes = (int32_t)at.sharedSizeBytes;
  if (vgprs) *vgprs = at.numRegs;
  return 0;
}

}  // extern "C"
