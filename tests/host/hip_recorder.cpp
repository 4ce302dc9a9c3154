// The stand-in HIP runtime of the host walk (hip_recorder.h).  Linked instead of libamdhip64: no device, no allocation.
#include "hip_recorder.h"

#include <cxxabi.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>

namespace rec {

long total_launches = 0, total_attrs = 0;

namespace {
struct Kernel {
    std::string name;
    std::vector<int> kinds;
};
std::map<const void*, Kernel>& kernels() {      // filled by static constructors of the library's objects: built on first use
    static std::map<const void*, Kernel> k;
    return k;
}
std::map<std::string, int>& lds_limits() {         // kernel -> the largest MaxDynamicSharedMemorySize set so far in this process
    static std::map<std::string, int> m;
    return m;
}
struct State {
    std::vector<Launch> launches;
    std::vector<Attr> attrs;
    std::vector<Arena> arenas;
    int fail_at = -1, fail_code = 0, after_failure = 0;
    bool failure_seen = false;
    int pending_error = 0;
    dim3 cfg_grid, cfg_block;
    size_t cfg_lds = 0;
    hipStream_t cfg_stream = nullptr;
};
State& st() {
    static State s;
    return s;
}

// the kinds of a demangled kernel's parameters: the last top-level (...) group, split at top-level commas
std::vector<int> param_kinds(const std::string& dem) {
    std::vector<int> kinds;
    const size_t close = dem.rfind(')');
    if (close == std::string::npos) return kinds;
    int depth = 0;
    size_t open = std::string::npos;
    for (size_t i = close + 1; i-- > 0;) {
        const char c = dem[i];
        if (c == ')' || c == '>' || c == ']') ++depth;
        else if (c == '(' || c == '<' || c == '[') {
            if (--depth == 0) { open = i; break; }
        }
    }
    if (open == std::string::npos || close == open + 1) return kinds;
    static const char* scalars[] = {"bool", "char", "signed char", "unsigned char", "short", "unsigned short", "int", "unsigned int",
                                    "long", "unsigned long", "long long", "unsigned long long", "float", "double", "__bf16", "_Float16"};
    std::string cur;
    depth = 0;
    auto flush = [&]() {
        while (!cur.empty() && cur.back() == ' ') cur.pop_back();
        while (!cur.empty() && cur.front() == ' ') cur.erase(cur.begin());
        if (cur.size() > 6 && cur.compare(cur.size() - 6, 6, " const") == 0) cur.erase(cur.size() - 6);
        int kind = 2;
        if (!cur.empty() && cur.back() == '*') kind = 1;
        else
            for (const char* s : scalars)
                if (cur == s) kind = 0;
        kinds.push_back(kind);
        cur.clear();
    };
    for (size_t i = open + 1; i < close; ++i) {
        const char c = dem[i];
        if (c == '<' || c == '(' || c == '[') ++depth;
        if (c == '>' || c == ')' || c == ']') --depth;
        if (c == ',' && depth == 0) flush();
        else cur.push_back(c);
    }
    flush();
    return kinds;
}
}  // namespace

bool Launch::operator==(const Launch& o) const {
    return kernel == o.kernel && memcmp(grid, o.grid, sizeof grid) == 0 && memcmp(block, o.block, sizeof block) == 0 && lds == o.lds &&
           stream == o.stream && kinds == o.kinds && ptrs == o.ptrs;
}

void reset() {
    State& s = st();
    s.launches.clear();
    s.attrs.clear();
    s.arenas.clear();
    s.fail_at = -1;
    s.after_failure = 0;
    s.failure_seen = false;
    s.pending_error = 0;
}

void* arena(const char* name, int64_t bytes, int misalign) {
    State& s = st();
    // 2^44 + k 2^40: a terabyte apart, far from anything the process maps, never dereferenced
    const uintptr_t lo = ((uintptr_t)1 << 44) + ((uintptr_t)(s.arenas.size() + 1) << 40) + (uintptr_t)misalign;
    s.arenas.push_back({name, lo, bytes > 0 ? (uint64_t)bytes : 0});
    return (void*)lo;
}

const std::vector<Launch>& launches() { return st().launches; }
const std::vector<Attr>& attrs() { return st().attrs; }
const std::vector<Arena>& arenas() { return st().arenas; }
void fail_launch(int k, int code) {
    st().fail_at = k;
    st().fail_code = code;
}
int launches_after_failure() { return st().after_failure; }

std::string describe(const Launch& l) {
    char buf[256];
    snprintf(buf, sizeof buf, " grid %u %u %u block %u %u %u lds %zu", l.grid[0], l.grid[1], l.grid[2], l.block[0], l.block[1],
             l.block[2], l.lds);
    return l.kernel + buf;
}

std::string check_call() {
    const State& s = st();
    for (size_t i = 0; i < s.launches.size(); ++i) {
        const Launch& l = s.launches[i];
        const std::string at = "launch " + std::to_string(i) + " " + describe(l) + ": ";
        if (l.grid[0] < 1 || l.grid[0] > 0x7fffffffu) return at + "grid.x outside 1..2^31-1";
        if (l.grid[1] < 1 || l.grid[1] > 65535 || l.grid[2] < 1 || l.grid[2] > 65535) return at + "grid.y / grid.z outside 1..65535";
        const uint64_t threads = (uint64_t)l.block[0] * l.block[1] * l.block[2];
        if (threads == 0 || threads % 64 != 0 || threads > 1024) return at + "block not a multiple of 64 in 64..1024";
        if (l.lds > 163840) return at + "dynamic LDS above 163840 B";
        if (l.lds > 65536) {
            // the library raises a kernel's limit once per process (a static flag), so the limits outlive reset()
            auto it = lds_limits().find(l.kernel);
            if (it == lds_limits().end() || (size_t)it->second < l.lds) return at + "dynamic LDS above 65536 B without hipFuncSetAttribute";
        }
        for (size_t p = 0; p < l.ptrs.size(); ++p) {
            if (l.kinds[p] != 1 || l.ptrs[p] == 0) continue;
            bool inside = false;
            for (const Arena& a : s.arenas)
                if (l.ptrs[p] >= a.lo && l.ptrs[p] - a.lo < a.bytes) inside = true;
            if (!inside) {
                char buf[96];
                snprintf(buf, sizeof buf, "pointer parameter %zu = 0x%llx outside every arena", p, (unsigned long long)l.ptrs[p]);
                return at + buf;
            }
        }
    }
    return "";
}

}  // namespace rec

// ------------------------------------------------------------------------------------------------ the 13 symbols
using rec::st;

extern "C" {

void** __hipRegisterFatBinary(const void*) {
    static void* module[1];
    return module;
}
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* hostFunction, char*, const char* deviceName, unsigned int, void*, void*, void*, void*,
                           int*) {
    int status = 0;
    char* dem = abi::__cxa_demangle(deviceName, nullptr, nullptr, &status);
    rec::Kernel k;
    k.name = (status == 0 && dem) ? dem : deviceName;
    free(dem);
    k.kinds = rec::param_kinds(k.name);
    rec::kernels()[hostFunction] = k;
}

hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
    st().cfg_grid = grid;
    st().cfg_block = block;
    st().cfg_lds = lds;
    st().cfg_stream = stream;
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
    *grid = st().cfg_grid;
    *block = st().cfg_block;
    *lds = st().cfg_lds;
    *stream = st().cfg_stream;
    return hipSuccess;
}

hipError_t hipLaunchKernel(const void* func, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t stream) {
    rec::State& s = st();
    rec::Launch l;
    auto it = rec::kernels().find(func);
    if (it == rec::kernels().end()) {
        fprintf(stderr, "hip_recorder: launch of an unregistered kernel %p\n", func);
        abort();
    }
    l.kernel = it->second.name;
    l.kinds = it->second.kinds;
    l.grid[0] = grid.x, l.grid[1] = grid.y, l.grid[2] = grid.z;
    l.block[0] = block.x, l.block[1] = block.y, l.block[2] = block.z;
    l.lds = lds;
    l.stream = stream;
    for (size_t p = 0; p < l.kinds.size(); ++p) {
        uintptr_t v = 0;
        if (l.kinds[p] == 1) memcpy(&v, args[p], sizeof v);
        l.ptrs.push_back(v);
    }
    const int index = (int)s.launches.size();
    l.failed = index == s.fail_at;
    if (s.failure_seen) ++s.after_failure;
    s.launches.push_back(l);
    ++rec::total_launches;
    if (l.failed) {
        s.failure_seen = true;
        s.pending_error = s.fail_code;
        return (hipError_t)s.fail_code;
    }
    return hipSuccess;
}

hipError_t hipGetLastError(void) {
    const int e = st().pending_error;
    st().pending_error = 0;
    return (hipError_t)e;
}
const char* hipGetErrorString(hipError_t) { return "recorded error"; }

hipError_t hipFuncSetAttribute(const void* func, hipFuncAttribute attr, int value) {
    auto it = rec::kernels().find(func);
    st().attrs.push_back({it == rec::kernels().end() ? std::string("?") : it->second.name, (int)attr, value});
    ++rec::total_attrs;
    if (attr == hipFuncAttributeMaxDynamicSharedMemorySize && it != rec::kernels().end()) {
        int& lim = rec::lds_limits()[it->second.name];
        if (value > lim) lim = value;
    }
    return hipSuccess;
}

hipError_t hipEventCreate(hipEvent_t* e) {
    *e = (hipEvent_t)malloc(1);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    free((void*)e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
    *ms = 0.f;
    return hipSuccess;
}

}  // extern "C"
