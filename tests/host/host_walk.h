// The table machinery of the host walk: an entry of include/drn.h gets a parameter block with a valid default, a function that
// builds the arenas and makes the call, and a list of single changes - each either still valid (DRN_OK, legal launches) or one
// documented refusal (DRN_EINVAL, nothing launched, no attribute call).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "drn.h"
#include "hip_recorder.h"

namespace hw {

extern bool list_only;                 // --list: entries are named, nothing is called
extern bool verbose;
extern void* const STREAM;             // the stream every call is given (a fake handle; recorded with each launch)

struct Tally {
    long entries = 0, cases = 0, ok_calls = 0, refusals = 0, injected = 0, host_only = 0;
};
extern Tally tally;

// one arena of the next call moved off its grid by name: the way a case misaligns ONE operand of a clause that checks several
extern const char* off_name;
extern int off_bytes;
inline void off(const char* name, int bytes) { off_name = name, off_bytes = bytes; }
inline void* A(const char* name, int64_t bytes, int misalign = 0) {
    return rec::arena(name, bytes, misalign + (off_name && std::string(off_name) == name ? off_bytes : 0));
}

[[noreturn]] void fail(const std::string& what);
void begin_entry(const char* name);    // counts (and with --list prints) a launching entry
void case_line(const std::string& label, const char* outcome, size_t launches);

// a call that must succeed with at least `min_launches` legal launches (0: a documented no-op)
void expect_ok(const std::string& label, const std::function<int()>& fn, int min_launches = 1);
// a call that must be refused: DRN_EINVAL, zero launches, zero attribute calls
void expect_refusal(const std::string& label, const std::function<int()>& fn);
// either of the two, whichever the library chooses - but never a half: OK with legal launches, or EINVAL with none (section D)
int expect_ok_or_refusal(const std::string& label, const std::function<int()>& fn);

template <class P>
struct Change {
    const char* what;
    std::function<void(P&)> apply;
};

// `call` makes the arenas itself (rec::reset() has been called) and returns the entry's code
template <class P>
void entry(const char* name, int (*call)(const P&), const std::vector<Change<P>>& refusals, const std::vector<Change<P>>& valid = {},
           const std::vector<Change<P>>& either = {}) {
    begin_entry(name);
    if (list_only) return;
    const std::string n = name;
    expect_ok(n + ": base", [&] { return call(P()); });
    // an entry of several launches stops at the first that fails, with its code (one launch: the code comes back)
    const size_t launches = rec::launches().size();
    for (size_t k = 0; k < launches; ++k) {
        rec::reset();
        rec::fail_launch((int)k, 700 + (int)k);
        const int rc = call(P());
        if (rc != 700 + (int)k) fail(n + ": launch " + std::to_string(k) + " failed with " + std::to_string(700 + k) + ", the call returns " + std::to_string(rc));
        if (rec::launches_after_failure() != 0) fail(n + ": a launch behind the failed launch " + std::to_string(k));
        ++tally.injected;
    }
    for (const auto& c : valid) {
        P p;
        off(nullptr, 0);
        c.apply(p);
        expect_ok(n + ": " + c.what, [&] { return call(p); }, 0);
    }
    for (const auto& c : refusals) {
        P p;
        off(nullptr, 0);
        c.apply(p);
        expect_refusal(n + ": " + c.what, [&] { return call(p); });
    }
    for (const auto& c : either) {
        P p;
        off(nullptr, 0);
        c.apply(p);
        expect_ok_or_refusal(n + ": " + c.what, [&] { return call(p); });
    }
    off(nullptr, 0);
}

#define CH(P, what, stmt) hw::Change<P>{what, [](P& p) { stmt; }}

// the families (host_walk_*.cpp)
void family_elementwise();
void family_pictures();
void family_gemm();
void family_attention();
void family_vae();
void family_forward();
void family_host_only();
void gemm_plan_cases(const char* path);       // section B: the golden's cases, handed over as text

}  // namespace hw
