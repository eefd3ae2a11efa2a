// runtime.cpp -- the shared state of the host runtime: devices and their
// modules, the hiprtc code-object cache, workspaces, launches, device error
// words, the timing pool.
#include "wx_host.hpp"

#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <fstream>
#include <map>
#include <thread>

namespace wx {

// g_mu guards the shared maps (devices and their modules, workspaces) and
// the timing-event pool; it is never held across a compile or a device
// synchronisation, so host threads driving different devices
// (multi_gpu.cpp) run concurrently.
std::recursive_mutex g_mu;
using Lock = std::lock_guard<std::recursive_mutex>;
std::atomic<int64_t> g_compiles{0}, g_hits{0};

std::map<int, DeviceState> g_devices;
std::map<std::pair<int, hipStream_t>, std::unique_ptr<Workspace>> g_ws;

struct TimedLaunch {
  hipEvent_t a, b;
  int device;
};
// the WX_F_TIME launches of the process not yet read (any thread: the C++
// multi-GPU path launches from one host thread per device), under g_mu
std::vector<TimedLaunch> g_timed;
std::map<int, std::vector<hipEvent_t>> g_event_pool;  // per device

// Grow a workspace buffer.  Every fill of a workspace buffer is ordered on
// the workspace's own stream: the kernels that rely on zeroed look-back words
// and tickets run there, and torch's pool streams are non-blocking, so a
// null-stream hipMemset is not ordered before them (hipMemset returns before
// the fill lands: tools/memset_order_probe.hip).  hipFree
// synchronises the device, so no in-flight kernel still uses the old buffer.
void ensure(Workspace &w, Buf &b, size_t bytes, bool zero) {
  if (b.bytes >= bytes && b.p) return;
  if (b.p) WX_HIP(hipFree(b.p));
  b.p = nullptr;
  b.bytes = 0;
  size_t want = std::max<size_t>(bytes, 256);
  WX_HIP(hipMalloc(&b.p, want));
  if (std::find(w.bufs.begin(), w.bufs.end(), &b) == w.bufs.end()) w.bufs.push_back(&b);
  if (zero) WX_HIP(hipMemsetAsync(b.p, 0, want, w.stream));
  b.bytes = want;
}

DeviceState &device_state(int dev, bool need_device) {
  Lock lk(g_mu);
  auto it = g_devices.find(dev);
  if (it != g_devices.end() && (!need_device || !it->second.arch.empty())) return it->second;
  DeviceState &d = g_devices[dev];
  if (need_device) {
    hipDeviceProp_t prop;
    WX_HIP(hipGetDeviceProperties(&prop, dev));
    d.arch = prop.gcnArchName;
    d.cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  return d;
}

Workspace &workspace(int dev, hipStream_t s) {
  Lock lk(g_mu);
  auto key = std::make_pair(dev, s);
  auto it = g_ws.find(key);
  if (it != g_ws.end()) return *it->second;
  auto w = std::make_unique<Workspace>();
  w->device = dev;
  w->stream = s;
  ensure(*w, w->ctrs, 64, true);
  Workspace &ref = *w;
  g_ws.emplace(key, std::move(w));
  return ref;
}

// The workspace of (dev, s) if an operation has opened one, else null: no
// device call, so a report of host-side state works where no device is.
Workspace *find_workspace(int dev, hipStream_t s) {
  Lock lk(g_mu);
  auto it = g_ws.find(std::make_pair(dev, s));
  return it == g_ws.end() ? nullptr : it->second.get();
}

uint64_t fnv1a(const std::string &s) {
  uint64_t h = 1469598103934665603ull;
  for (unsigned char c : s) {
    h ^= c;
    h *= 1099511628211ull;
  }
  return h;
}

// Code-object cache: $WARPDB_KERNEL_CACHE, or .kernel_cache next to this
// library (so objects built in one container travel with the tree); "off"
// disables it.
std::string cache_dir() {
  std::string d = env_or("WARPDB_KERNEL_CACHE", "");
  if (d == "off" || d == "0") return std::string();
  if (d.empty()) {
    Dl_info info;
    if (dladdr(reinterpret_cast<void *>(&wx_abi_version), &info) && info.dli_fname) {
      std::string lib = info.dli_fname;
      auto slash = lib.find_last_of('/');
      d = (slash == std::string::npos ? std::string(".") : lib.substr(0, slash)) + "/.kernel_cache";
    }
  }
  return d;
}

void mkdirs(const std::string &d) {
  std::string cur;
  for (size_t i = 0; i < d.size(); ++i) {
    cur += d[i];
    if (d[i] == '/' && cur.size() > 1) mkdir(cur.c_str(), 0755);
  }
  mkdir(d.c_str(), 0755);
}

// Identity of the compiler behind the code-object cache: the hiprtc version
// and the ROCm build string of the installation it comes from.
const std::string &compiler_id() {
  static const std::string id = [] {
    int major = 0, minor = 0;
    (void)hiprtcVersion(&major, &minor);
    std::string v = "hiprtc " + std::to_string(major) + "." + std::to_string(minor);
    std::ifstream in(env_or("ROCM_PATH", "/opt/rocm") + "/.info/version");
    std::string rocm;
    if (in && std::getline(in, rocm)) v += " rocm " + rocm;
    return v;
  }();
  return id;
}

// Compile with hiprtc.  Options: gfx950 (the device's full target id),
// -O3, no FP contraction (projections stay bit-identical to the CPU
// evaluator), hardware f64 atomics.
std::vector<char> compile_program(const std::string &src, const std::string &arch) {
  const std::string arch_opt = "--offload-arch=" + arch;
  std::vector<const char *> opts = {arch_opt.c_str(), "-O3", "-std=c++17", "-ffp-contract=off",
                                    "-munsafe-fp-atomics"};
  const std::string dir = cache_dir();
  std::string path;
  if (!dir.empty()) {
    std::string keysrc = src;
    for (auto o : opts) keysrc += std::string("\x01") + o;
    keysrc += std::string("\x01") + compiler_id();  // a cached object from another hiprtc is never reused
    char name[64];
    std::snprintf(name, sizeof(name), "%016llx-%zu.co", (unsigned long long)fnv1a(keysrc), src.size());
    path = dir + "/" + name;
    std::ifstream in(path, std::ios::binary);
    if (in) {
      std::vector<char> code((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
      if (!code.empty()) return code;
    }
  }
  hiprtcProgram prog = nullptr;
  if (hiprtcCreateProgram(&prog, src.c_str(), "warpexec_query.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
    fail(WX_ERR_COMPILE, "HIPRTC error: hiprtcCreateProgram failed");
  struct Guard {
    hiprtcProgram p;
    ~Guard() {
      if (p) hiprtcDestroyProgram(&p);
    }
  } guard{prog};
  hiprtcResult r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
  size_t log_size = 0;
  hiprtcGetProgramLogSize(prog, &log_size);
  std::string log(log_size, '\0');
  if (log_size) hiprtcGetProgramLog(prog, &log[0]);
  if (r != HIPRTC_SUCCESS)
    fail(WX_ERR_COMPILE, std::string("Kernel compilation failed.\n") + hiprtcGetErrorString(r) + "\n" + log);
  size_t code_size = 0;
  if (hiprtcGetCodeSize(prog, &code_size) != HIPRTC_SUCCESS || !code_size)
    fail(WX_ERR_COMPILE, "HIPRTC error: empty code object");
  std::vector<char> code(code_size);
  hiprtcGetCode(prog, code.data());
  ++g_compiles;
  if (!path.empty()) {
    mkdirs(dir);
    std::string tmp = path + ".tmp" + std::to_string(getpid()) + "." +
                      std::to_string(std::hash<std::thread::id>()(std::this_thread::get_id()));
    {
      std::ofstream out(tmp, std::ios::binary);
      out.write(code.data(), (std::streamsize)code.size());
    }
    std::rename(tmp.c_str(), path.c_str());
  }
  return code;
}

std::shared_ptr<Module> get_module(int dev, const Spec &spec, bool load) {
  const std::string key = spec.key_string();
  std::string arch;
  {
    Lock lk(g_mu);
    DeviceState &d = device_state(dev, load);
    auto it = d.modules.find(key);
    if (it != d.modules.end() && (!load || it->second->mod)) {
      ++g_hits;
      return it->second;
    }
    arch = d.arch.empty() ? default_arch() : d.arch;
  }
  // compile and load outside the lock; if another thread got there first,
  // keep its module
  const int64_t compiles_before = g_compiles;
  std::vector<char> code = compile_program(spec.source(), arch);
  if (g_compiles != compiles_before && std::getenv("WARPDB_DEBUG"))  // a code-object cache miss
    std::fprintf(stderr, "[warpexec] hiprtc compile (cache miss): %s\n", key.substr(0, 300).c_str());
  auto m = std::make_shared<Module>();
  if (load) WX_HIP(hipModuleLoadData(&m->mod, code.data()));
  if (!load) return m;
  Lock lk(g_mu);
  DeviceState &d = device_state(dev, load);
  auto it = d.modules.find(key);
  if (it != d.modules.end() && it->second->mod) {
    (void)hipModuleUnload(m->mod);
    return it->second;
  }
  d.modules[key] = m;
  return m;
}

bool device_visible(const wx_launch &L) {
  int ndev = 0;
  return hipGetDeviceCount(&ndev) == hipSuccess && ndev > L.device;
}

// The module of a prepare call: loaded where the launch's device is visible,
// compiled only (into the code-object cache) where it is not.
void prepare_module(const wx_launch &L, const Spec &spec) {
  if (device_visible(L)) {
    DevGuard g(L.device);
    get_module(L.device, spec, true);
  } else {
    get_module(L.device, spec, false);
  }
}

void launch(hipFunction_t f, unsigned grid, void *args, hipStream_t s, bool timed, unsigned block, unsigned shmem) {
  void *params[] = {args};
  hipEvent_t ea = nullptr, eb = nullptr;
  int dev = 0;
  if (timed) {
    WX_HIP(hipGetDevice(&dev));
    auto take = [dev](hipEvent_t &e) {
      Lock lk(g_mu);
      auto &pool = g_event_pool[dev];  // events belong to the device they were created on
      if (!pool.empty()) {
        e = pool.back();
        pool.pop_back();
      } else {
        // timing only: no system-scope fence (cache writeback + invalidate)
        // when the event is recorded, so timing a launch does not slow the
        // stream it times
        WX_HIP(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
      }
    };
    take(ea);
    take(eb);
    WX_HIP(hipEventRecord(ea, s));
  }
  WX_HIP(hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, shmem, s, params, nullptr));
  if (timed) {
    WX_HIP(hipEventRecord(eb, s));
    Lock lk(g_mu);
    g_timed.push_back({ea, eb, dev});
  }
}

// Read (and clear) device error bits of a workspace; throws on any.
std::string lookback_report(const uint64_t *d) {
  // d = ctrs[3..7]: claim, {kind | launch epoch << 8 | digit << 16 | pass << 32}, waiting tile,
  // waited-on tile, the status word seen (wx_args.h WX_LBD_*)
  if (!d[0]) return " (no report recorded)";
  const unsigned kind = (unsigned)(d[1] & 0xff), epoch = (unsigned)((d[1] >> 8) & 0xff);
  const unsigned digit = (unsigned)((d[1] >> 16) & 0xffff), pass = (unsigned)(d[1] >> 32);
  const unsigned seen_epoch = (unsigned)(d[4] >> 58), seen_flag = (unsigned)((d[4] >> 56) & 3);
  char b[320];
  if (kind == WX_LBD_RADIX)
    std::snprintf(b, sizeof b,
                  ": radix pass %u tile %llu digit %u waited on tile %llu, whose word 0x%016llx has epoch %u flag %u "
                  "(launch epoch %u)",
                  pass, (unsigned long long)d[2], digit, (unsigned long long)d[3], (unsigned long long)d[4],
                  seen_epoch, seen_flag, epoch);
  else
    std::snprintf(b, sizeof b,
                  ": compaction tile %llu waited on tile %llu, whose word 0x%016llx has epoch %u flag %u "
                  "(launch epoch %u)",
                  (unsigned long long)d[2], (unsigned long long)d[3], (unsigned long long)d[4], seen_epoch, seen_flag,
                  epoch);
  return b;
}

void check_errors(Workspace &w) {
  // both error words (and the look-back report) through one pinned buffer
  // and one stream sync (pageable synchronous copies cost ≈ 10 µs each)
  if (!w.h_err) WX_HIP(hipHostMalloc(reinterpret_cast<void **>(&w.h_err), 8 * sizeof(uint64_t)));
  for (int i = 0; i < 8; ++i) w.h_err[i] = 0;
  // h_err[0..6] = ctrs[1..7], h_err[7] = g_ctrs[1]
  WX_HIP(hipMemcpyAsync(&w.h_err[0], static_cast<uint64_t *>(w.ctrs.p) + 1, 7 * 8, hipMemcpyDeviceToHost, w.stream));
  if (w.g_ctrs.p)
    WX_HIP(hipMemcpyAsync(&w.h_err[7], static_cast<uint64_t *>(w.g_ctrs.p) + 1, 8, hipMemcpyDeviceToHost, w.stream));
  WX_HIP(hipStreamSynchronize(w.stream));
  const uint64_t bits = w.h_err[0] | w.h_err[7];
  if (!bits) return;
  const std::string report = lookback_report(&w.h_err[2]);
  // clear on the workspace stream: ordered before the next launch that reads them
  WX_HIP(hipMemsetAsync(static_cast<uint64_t *>(w.ctrs.p) + 1, 0, 8, w.stream));
  WX_HIP(hipMemsetAsync(static_cast<uint64_t *>(w.ctrs.p) + WX_LBD_BASE, 0, 5 * 8, w.stream));
  if (w.g_ctrs.p) WX_HIP(hipMemsetAsync(static_cast<uint64_t *>(w.g_ctrs.p) + 1, 0, 8, w.stream));
  if (bits & WX_DEVERR_LOOKBACK) fail(WX_ERR_INTERNAL, "device look-back timed out (results invalid)" + report);
  if (bits & WX_DEVERR_CAPACITY) fail(WX_ERR_CAPACITY, "group table / output capacity exceeded");
  if (bits & WX_DEVERR_UNSUPPORTED)
    fail(WX_ERR_UNSUPPORTED, "more than 4096 distinct GROUP BY keys outside the dense key window");
  if (bits & WX_DEVERR_INTERNAL_KEY)
    fail(WX_ERR_INTERNAL, "GROUP BY consistency check failed (a key outside its planned range, a work-item "
                          "overflow, or row counts that disagree between passes)");
  if (bits & WX_DEVERR_JOIN_PROBE)
    fail(WX_ERR_INTERNAL, "JOIN: table consistency check failed (a probe walked the whole hash table without meeting an empty "
                          "slot, or the build met a key outside the key range it had found)");
  fail(WX_ERR_INTERNAL, "device error bits set");
}

// Where a call's count lands on the device: the caller's buffer, else (when
// one is needed) the 8-byte workspace slot `b`.
int64_t *count_slot(Workspace &w, Buf &b, int64_t *d_dst, bool need) {
  if (d_dst || !need) return d_dst;
  ensure(w, b, 8, false);
  return static_cast<int64_t *>(b.p);
}

// The end of a merge: the count read to the host through the workspace's
// landing word (true), or no read and WX_F_SYNC's synchronisation alone.
bool read_count(Op &op, const int64_t *d_src, int64_t *h_dst) {
  if (h_dst) {
    WX_HIP(hipMemcpyAsync(&op.w.host_word, d_src, 8, hipMemcpyDeviceToHost, op.s));
    WX_HIP(hipStreamSynchronize(op.s));
    *h_dst = (int64_t)op.w.host_word;
  } else if (op.L.flags & WX_F_SYNC) {
    WX_HIP(hipStreamSynchronize(op.s));
  }
  return h_dst != nullptr;
}

// The grid of a grid-stride kernel. per_cu, the workgroups per CU, is the
// per-op value measured best (profiles/r01/ablate_stream.txt).
unsigned grid_for(int64_t work_items, int cus, int per_cu) {
  int64_t g = (work_items + WX_BLOCK - 1) / WX_BLOCK;
  const int64_t cap = (int64_t)cus * per_cu;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// Sum and count of the unread timed launches of `device` (-1: every device).
void timing_take(int32_t device, double *total_ms, int64_t *launches) {
  std::vector<TimedLaunch> mine;
  {
    Lock lk(g_mu);
    auto keep = std::partition(g_timed.begin(), g_timed.end(),
                               [&](const TimedLaunch &t) { return device >= 0 && t.device != device; });
    mine.assign(keep, g_timed.end());
    g_timed.erase(keep, g_timed.end());
  }
  double tot = 0;
  int64_t n = 0;
  for (auto &tl : mine) {
    DevGuard g(tl.device);
    WX_HIP(hipEventSynchronize(tl.b));
    float ms = 0;
    WX_HIP(hipEventElapsedTime(&ms, tl.a, tl.b));
    tot += ms;
    ++n;
    Lock lk(g_mu);
    g_event_pool[tl.device].push_back(tl.a);
    g_event_pool[tl.device].push_back(tl.b);
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = n;
}

void cache_stats(int64_t *compiles, int64_t *hits) {
  if (compiles) *compiles = g_compiles;
  if (hits) *hits = g_hits;
}

void shutdown() {
  Lock lk(g_mu);
  for (auto &kv : g_ws) {
    Workspace &w = *kv.second;
    (void)hipSetDevice(w.device);
    // every buffer the workspace allocated (a fixed list here missed the
    // GROUP BY list / partition, exchange, row-order and fold buffers)
    for (Buf *b : w.bufs)
      if (b->p) (void)hipFree(b->p);
    if (w.h_err) (void)hipHostFree(w.h_err);
  }
  g_ws.clear();
  for (auto &kv : g_devices) {
    (void)hipSetDevice(kv.first);
    for (auto &m : kv.second.modules)
      if (m.second->mod) (void)hipModuleUnload(m.second->mod);
  }
  g_devices.clear();
  for (auto &kv : g_event_pool) {
    (void)hipSetDevice(kv.first);
    for (auto e : kv.second) (void)hipEventDestroy(e);
  }
  g_event_pool.clear();
  for (auto &t : g_timed) {
    (void)hipSetDevice(t.device);
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  g_timed.clear();
}

}  // namespace wx
