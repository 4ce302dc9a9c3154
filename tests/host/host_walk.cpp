// host_walk: libdrn's host half - argument checks, workspace carving, plans, grid arithmetic - run on the CPU against a recording
// stand-in for the HIP runtime, under ASan and UBSan.  One line per case, a tally at the end, non-zero exit on the first broken rule.
//   host_walk [--list] [--verbose] [--gemm-cases FILE]
#include "host_walk.h"

#include <string.h>

namespace hw {

bool list_only = false, verbose = false;
void* const STREAM = (void*)(uintptr_t)0x5717ea00;
Tally tally;
const char* off_name = nullptr;
int off_bytes = 0;

void fail(const std::string& what) {
    fflush(stdout);
    fprintf(stdout, "FAIL %s\n", what.c_str());
    fprintf(stderr, "host_walk: FAIL %s\n", what.c_str());
    exit(1);
}

void begin_entry(const char* name) {
    ++tally.entries;
    if (list_only) printf("%s\n", name);
}

void case_line(const std::string& label, const char* outcome, size_t launches) {
    ++tally.cases;
    printf("case %-88s %s launches %zu\n", label.c_str(), outcome, launches);
    if (verbose)
        for (const rec::Launch& l : rec::launches()) printf("    launch %s\n", rec::describe(l).c_str());
}

static void check_streams(const std::string& label) {
    for (const rec::Launch& l : rec::launches())
        if (l.stream != STREAM) fail(label + ": a launch on another stream than the caller's: " + rec::describe(l));
}

void expect_ok(const std::string& label, const std::function<int()>& fn, int min_launches) {
    rec::reset();
    const int rc = fn();
    if (rc != DRN_OK) fail(label + ": expected DRN_OK, got " + std::to_string(rc));
    if ((int)rec::launches().size() < min_launches) fail(label + ": DRN_OK with " + std::to_string(rec::launches().size()) + " launches");
    const std::string bad = rec::check_call();
    if (!bad.empty()) fail(label + ": " + bad);
    check_streams(label);
    ++tally.ok_calls;
    case_line(label, "OK    ", rec::launches().size());
}

void expect_refusal(const std::string& label, const std::function<int()>& fn) {
    rec::reset();
    const int rc = fn();
    if (rc != DRN_EINVAL) fail(label + ": expected DRN_EINVAL, got " + std::to_string(rc));
    if (!rec::launches().empty())
        fail(label + ": refused after " + std::to_string(rec::launches().size()) + " launches, first " + rec::describe(rec::launches()[0]));
    if (!rec::attrs().empty()) fail(label + ": refused after a hipFuncSetAttribute call");
    ++tally.refusals;
    case_line(label, "EINVAL", 0);
}

int expect_ok_or_refusal(const std::string& label, const std::function<int()>& fn) {
    rec::reset();
    const int rc = fn();
    if (rc == DRN_EINVAL) {
        if (!rec::launches().empty() || !rec::attrs().empty()) fail(label + ": refused after launching");
        ++tally.refusals;
        case_line(label, "EINVAL", 0);
    } else if (rc == DRN_OK) {
        const std::string bad = rec::check_call();
        if (!bad.empty()) fail(label + ": " + bad);
        check_streams(label);
        ++tally.ok_calls;
        case_line(label, "OK    ", rec::launches().size());
    } else {
        fail(label + ": expected DRN_OK or DRN_EINVAL, got " + std::to_string(rc));
    }
    return rc;
}

}  // namespace hw

int main(int argc, char** argv) {
    const char* gemm_cases = nullptr;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--list")) hw::list_only = true;
        else if (!strcmp(argv[i], "--verbose")) hw::verbose = true;
        else if (!strcmp(argv[i], "--gemm-cases") && i + 1 < argc) gemm_cases = argv[++i];
        else {
            fprintf(stderr, "usage: host_walk [--list] [--verbose] [--gemm-cases FILE]\n");
            return 2;
        }
    }
    if (gemm_cases && !hw::list_only) {          // section B under one process's settings (the A/B switches are read once)
        hw::gemm_plan_cases(gemm_cases);
        return 0;
    }
    hw::family_elementwise();
    hw::family_pictures();
    hw::family_gemm();
    hw::family_attention();
    hw::family_vae();
    hw::family_forward();
    if (hw::list_only) return 0;
    hw::family_host_only();
    printf("tally entries %ld cases %ld ok %ld refusals %ld injected %ld host_only %ld launches %ld attribute_calls %ld\n",
           hw::tally.entries, hw::tally.cases, hw::tally.ok_calls, hw::tally.refusals, hw::tally.injected, hw::tally.host_only,
           rec::total_launches, rec::total_attrs);
    return 0;
}
