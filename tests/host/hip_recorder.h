// A stand-in for the 13 HIP runtime symbols libdrn's host code needs: nothing runs, every launch is recorded.
// The library's device pointers are never dereferenced on the host, so operands are "arenas": named, disjoint ranges of fake
// addresses with exact byte sizes.  See DESIGN.md (host walk).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace rec {

struct Launch {
    std::string kernel;             // demangled, with its parameter list
    unsigned grid[3], block[3];
    size_t lds;                     // dynamic LDS bytes
    void* stream;
    std::vector<int> kinds;         // per parameter: 0 scalar, 1 pointer, 2 by-value struct (opaque)
    std::vector<uintptr_t> ptrs;    // per parameter: the pointer's value (0 for the other kinds)
    bool failed;                    // this launch was told to fail
    bool operator==(const Launch& o) const;
};

struct Attr {
    std::string kernel;
    int attr, value;
    bool operator==(const Attr& o) const { return kernel == o.kernel && attr == o.attr && value == o.value; }
};

struct Arena {
    std::string name;
    uintptr_t lo;
    uint64_t bytes;
};

// ---- one call's state
void reset();                                              // forget launches, attribute calls, arenas and the injected failure
void* arena(const char* name, int64_t bytes, int misalign = 0);   // a fresh range (bytes <= 0: empty, but not null); base 4096-aligned + misalign
const std::vector<Launch>& launches();
const std::vector<Attr>& attrs();
const std::vector<Arena>& arenas();
void fail_launch(int k, int code);                         // launch number k (0-based) of this call returns `code`; -1: none
int launches_after_failure();                              // launches recorded after the injected one

// ---- the rules of a recorded call; an empty string = no violation
// legal: grid.x in 1..2^31-1, grid.y/z in 1..65535, block a multiple of 64 and <= 1024, dynamic LDS <= 163840 B and above 65536 B
// only after a hipFuncSetAttribute on that kernel with at least that size; every pointer null or inside an arena of this call.
std::string check_call();
std::string describe(const Launch& l);

// counters over the whole program
extern long total_launches, total_attrs;

}  // namespace rec
