// jit_cache: hiprtc and the on-disk code-object cache behind every kernel compiled at run time (user_model.hpp: jit_load).
// hiprtc is loaded lazily (dlopen), from next to the HIP runtime the process already uses, so the library itself carries no
// link-time dependency on it.  Code objects are cached on disk by source hash ($BAYESFILT_CACHE_DIR, else .jit_cache next to the
// library); the callers cache the loaded functions in memory.
#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "elf_extent.hpp"
#include "user_model.hpp"

#ifndef BF_ARCH_NAME
#define BF_ARCH_NAME "gfx950"
#endif

namespace bf {

namespace {

// ---- hiprtc, resolved at first use
typedef struct _hiprtcProgram* hiprtcProgram;
struct Rtc {
  void* h = nullptr;
  int (*CreateProgram)(hiprtcProgram*, const char*, const char*, int, const char**, const char**) = nullptr;
  int (*CompileProgram)(hiprtcProgram, int, const char**) = nullptr;
  int (*GetProgramLogSize)(hiprtcProgram, size_t*) = nullptr;
  int (*GetProgramLog)(hiprtcProgram, char*) = nullptr;
  int (*GetCodeSize)(hiprtcProgram, size_t*) = nullptr;
  int (*GetCode)(hiprtcProgram, char*) = nullptr;
  int (*DestroyProgram)(hiprtcProgram*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  int (*Version)(int*, int*) = nullptr;
};
Rtc g_rtc;   // (filled under the callers' lock: user_model.hip serialises every build)

bool load_rtc(std::string& why) {
  if (g_rtc.h) return true;
  std::vector<std::string> cand;
  const char* forced = std::getenv("BAYESFILT_HIPRTC_LIB");   // when set: this library and no other
  if (forced && *forced) {
    cand.push_back(forced);
  } else {
    Dl_info info;
    if (dladdr(reinterpret_cast<void*>(&hipModuleLoadData), &info) && info.dli_fname) {  // next to the runtime in use
      std::string p(info.dli_fname);
      const size_t slash = p.rfind('/');
      if (slash != std::string::npos) cand.push_back(p.substr(0, slash + 1) + "libhiprtc.so");
    }
    cand.push_back("libhiprtc.so");
    cand.push_back("libhiprtc.so.7");
    cand.push_back("/opt/rocm/lib/libhiprtc.so");
  }
  for (const std::string& c : cand) {
    void* h = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) {
      const char* de = dlerror();  // ONE call: dlerror() clears the message it returns
      why += c + ": " + (de ? de : "?") + "; ";
      continue;
    }
#define BF_RTC_SYM(F_) *reinterpret_cast<void**>(&g_rtc.F_) = dlsym(h, "hiprtc" #F_)
    BF_RTC_SYM(CreateProgram); BF_RTC_SYM(CompileProgram); BF_RTC_SYM(GetProgramLogSize); BF_RTC_SYM(GetProgramLog);
    BF_RTC_SYM(GetCodeSize); BF_RTC_SYM(GetCode); BF_RTC_SYM(DestroyProgram); BF_RTC_SYM(GetErrorString); BF_RTC_SYM(Version);
#undef BF_RTC_SYM
    if (g_rtc.CreateProgram && g_rtc.CompileProgram && g_rtc.GetCodeSize && g_rtc.GetCode && g_rtc.DestroyProgram) {
      g_rtc.h = h;
      return true;
    }
    why += c + ": hiprtc entry points missing; ";
    dlclose(h);
  }
  return false;
}

uint64_t fnv1a(const std::string& s) {
  uint64_t h = 1469598103934665603ull;
  for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
  return h;
}

std::string cache_dir() {  // $BAYESFILT_CACHE_DIR, else .jit_cache next to this library
  const char* e = std::getenv("BAYESFILT_CACHE_DIR");
  std::string d;
  if (e && *e) {
    d = e;
  } else {
    Dl_info info;
    d = ".";
    if (dladdr(reinterpret_cast<void*>(&bf::set_error), &info) && info.dli_fname) {
      const std::string p(info.dli_fname);
      const size_t slash = p.rfind('/');
      if (slash != std::string::npos) d = p.substr(0, slash);
    }
    d += "/.jit_cache";
  }
  mkdir(d.c_str(), 0755);
  return d;
}

bool read_file(const std::string& path, std::vector<char>& code) {
  code.clear();
  if (FILE* f = std::fopen(path.c_str(), "rb")) {
    std::fseek(f, 0, SEEK_END);
    const long sz = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (sz > 0) {
      code.resize((size_t)sz);
      if (std::fread(code.data(), 1, (size_t)sz, f) != (size_t)sz) code.clear();
    }
    std::fclose(f);
  }
  return !code.empty();
}

// every rank of a torchrun job misses at the same moment: each writes its OWN temporary (pid + counter) and renames it over
// the final name -- rename is atomic, a reader sees either nothing or a whole file
void write_file_atomically(const std::string& path, const std::vector<char>& code) {
  static std::atomic<unsigned> counter{0};
  const std::string tmp = path + "." + std::to_string((long long)getpid()) + "." + std::to_string(counter.fetch_add(1)) + ".tmp";
  if (FILE* f = std::fopen(tmp.c_str(), "wb")) {  // best effort
    const bool ok = std::fwrite(code.data(), 1, code.size(), f) == code.size();
    const bool closed = std::fclose(f) == 0;
    if (ok && closed && std::rename(tmp.c_str(), path.c_str()) == 0) return;
    std::remove(tmp.c_str());
  }
}

int compile_with_hiprtc(const std::string& src, std::vector<char>& code, bool contract_off) {
  std::string why;
  if (!load_rtc(why)) return set_error(BF_EUNSUPPORTED, "hiprtc is not available: %.400s", why.c_str());
  hiprtcProgram prog = nullptr;
  int rc = g_rtc.CreateProgram(&prog, src.c_str(), "bf_user_model.hip", 0, nullptr, nullptr);
  if (rc != 0) return set_error(BF_EHIP, "hiprtcCreateProgram failed (%d)", rc);
  // (contract_off = false: the translation unit keeps hipcc's default contraction -- what the ahead-of-time build of the same
  // kernel was compiled with -- and the source itself switches contraction off around the caller's functions)
  const char* opts[] = {"--offload-arch=" BF_ARCH_NAME, "-O3", "-std=c++17", "-ffp-contract=off"};
  rc = g_rtc.CompileProgram(prog, contract_off ? 4 : 3, opts);
  if (rc != 0) {
    size_t ls = 0;
    std::string log;
    if (g_rtc.GetProgramLogSize && g_rtc.GetProgramLogSize(prog, &ls) == 0 && ls > 1) {
      log.resize(ls);
      g_rtc.GetProgramLog(prog, &log[0]);
    }
    g_rtc.DestroyProgram(&prog);
    // the first error lines are what the author of the source needs
    const size_t pos = log.find("error");
    return set_error(BF_EINVAL, "the model source does not compile: %.440s", (pos == std::string::npos ? log : log.substr(pos)).c_str());
  }
  size_t cs = 0;
  rc = g_rtc.GetCodeSize(prog, &cs);
  if (rc == 0 && cs > 0) {
    code.resize(cs);
    rc = g_rtc.GetCode(prog, code.data());
  }
  g_rtc.DestroyProgram(&prog);
  if (rc != 0 || code.empty()) return set_error(BF_EHIP, "hiprtc returned no code object (%d)", rc);
  return BF_OK;
}

}  // namespace

// the code object depends on the source, the target and the compiler: all three are in the key (the HIP runtime's version
// stands for hiprtc's, which ships with it -- known without loading hiprtc on a cache hit)
std::string jit_source_key(const std::string& src) {
  int rtver = 0;
  (void)hipRuntimeGetVersion(&rtver);
  char key[32];
  std::snprintf(key, sizeof(key), "%016llx", (unsigned long long)fnv1a(src + "|" BF_ARCH_NAME "|" + std::to_string(rtver)));
  return key;
}

int jit_load(const std::string& src, std::initializer_list<std::pair<const char*, hipFunction_t*>> entries, bool contract_off, hipModule_t* mod_out) {
  const std::string path = cache_dir() + "/user_" + jit_source_key(src) + "_" BF_ARCH_NAME ".co";
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) {
    dev = -1;
    (void)hipGetLastError();
  }
  std::vector<char> code;
  hipModule_t mod = nullptr;
  hipError_t e = hipErrorUnknown;
  auto load = [&]() {
    hipError_t le = hipModuleLoadData(&mod, code.data());
    for (const auto& en : entries)
      if (le == hipSuccess) le = hipModuleGetFunction(en.second, mod, en.first);
    if (le != hipSuccess && mod) {
      (void)hipModuleUnload(mod);
      mod = nullptr;
    }
    return le;
  };
  if (read_file(path, code)) {
    e = elf_image_is_whole(code.data(), code.size()) ? load() : hipErrorInvalidImage;   // (elf_extent.hpp: the loader takes no length)
    if (e != hipSuccess) {   // a file that does not load -- truncated, stale, foreign -- is deleted and rebuilt
      (void)hipGetLastError();
      if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || dev < 0)
        return set_error(BF_ENOGPU, "loading the compiled model failed: %s", hipGetErrorString(e));
      std::remove(path.c_str());
      code.clear();
    }
  }
  if (code.empty()) {
    const int rc = compile_with_hiprtc(src, code, contract_off);
    if (rc != BF_OK) return rc;
    write_file_atomically(path, code);
    e = load();
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return set_error(e == hipErrorNoDevice ? BF_ENOGPU : BF_EHIP, "loading the compiled model failed: %s", hipGetErrorString(e));
  }
  if (mod_out) *mod_out = mod;
  return BF_OK;
}

}  // namespace bf
