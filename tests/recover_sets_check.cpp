// The host side of the recovery's index sets (lambdaworks_kzg_amd/csrc/recover_sets.h) as a stand-alone program, built under
// AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_recover_mixed_cpu.py. Every case prints one line, "<name> ok" or
// "<name> FAILED: ..."; the exit status is the number of failures.
#include <stdio.h>

#include <string>
#include <vector>

#include "recover_sets.h"

using namespace lwk;

namespace {

int failures = 0;

void report(const char *name, bool ok, const std::string &why = "") {
    if (!ok) failures++;
    printf("%s %s%s\n", name, ok ? "ok" : "FAILED: ", ok ? "" : why.c_str());
}

uint32_t rev7(uint32_t k) {
    uint32_t q = 0;
    for (int b = 0; b < 7; b++) q |= ((k >> b) & 1u) << (6 - b);
    return q;
}

// the lists one after the other in heap blocks of exactly their size, so that a read past either end is the sanitizer's
struct Lists {
    std::vector<uint64_t> idx;
    std::vector<size_t> num;
    void add(const std::vector<uint64_t> &l) {
        idx.insert(idx.end(), l.begin(), l.end());
        num.push_back(l.size());
    }
    bool run(RecoverSets &out) {
        std::vector<uint64_t> exact_idx(idx);   // (capacity == size)
        std::vector<size_t> exact_num(num);
        exact_idx.shrink_to_fit();
        exact_num.shrink_to_fit();
        return recover_sets_of(out, exact_idx.data(), exact_num.data(), exact_num.size());
    }
};

std::vector<uint64_t> range(uint64_t from, uint64_t to, uint64_t step = 1) {
    std::vector<uint64_t> l;
    for (uint64_t k = from; k < to; k += step) l.push_back(k);
    return l;
}

// does `set` describe exactly the list l?
bool set_is(const RecoverSet &set, const std::vector<uint64_t> &l) {
    uint32_t given[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < l.size(); i++) {
        if (set.k[i] != l[i]) return false;
        const uint32_t q = rev7((uint32_t)l[i]);
        given[q >> 5] |= 1u << (q & 31u);
    }
    for (size_t i = l.size(); i < kRecoverCells; i++)
        if (set.k[i] != 0) return false;
    return !memcmp(given, set.given, sizeof given);
}

void deduplication() {
    const std::vector<uint64_t> a = range(0, 128, 2), b = range(0, 100);
    Lists l;
    l.add(a);
    l.add(b);
    l.add(a);
    RecoverSets s;
    bool ok = l.run(s) && s.fault == kRecoverListGood && s.sets.size() == 2 && s.set_of == std::vector<uint32_t>({0, 1, 0});
    ok = ok && set_is(s.sets[0], a) && set_is(s.sets[1], b) && s.cell_off == std::vector<size_t>({0, 64, 164, 228});
    report("deduplication [A, B, A]", ok);
    // first occurrence decides the order, whatever the masks compare as
    Lists m;
    m.add(b);
    m.add(a);
    m.add(b);
    m.add(a);
    ok = m.run(s) && s.sets.size() == 2 && s.set_of == std::vector<uint32_t>({0, 1, 0, 1}) && set_is(s.sets[0], b) && set_is(s.sets[1], a);
    report("deduplication [B, A, B, A]", ok);
}

void offsets() {
    Lists l;
    l.add(range(0, 64));
    l.add(range(0, 128));
    l.add(range(63, 128));
    RecoverSets s;
    const bool ok = l.run(s) && s.sets.size() == 3 && s.set_of == std::vector<uint32_t>({0, 1, 2}) &&
                    s.cell_off == std::vector<size_t>({0, 64, 192, 257}) && set_is(s.sets[2], range(63, 128));
    report("offsets 64, 128, 65", ok);
}

// a good list, the faulty one, a good list: blob 1 is named, with the fault's kind and place
void fault(const char *name, const std::vector<uint64_t> &bad, RecoverListFault kind, size_t at) {
    Lists l;
    l.add(range(0, 64));
    l.add(bad);
    l.add(range(64, 128));
    RecoverSets s;
    const bool ok = !l.run(s) && s.fault == kind && s.bad_blob == 1 && (kind == kRecoverListCount || s.bad_at == at);
    report(name, ok, "fault " + std::to_string((int)s.fault) + " blob " + std::to_string(s.bad_blob) + " at " + std::to_string(s.bad_at));
    // and alone in front: blob 0
    Lists f;
    f.add(bad);
    f.add(range(0, 64));
    report((std::string(name) + " in front").c_str(), !f.run(s) && s.fault == kind && s.bad_blob == 0);
}

void faults() {
    fault("count 63", range(0, 63), kRecoverListCount, 0);
    fault("count 129", range(0, 129), kRecoverListCount, 0);
    std::vector<uint64_t> l = range(0, 64);
    l[63] = 128;
    fault("index 128", l, kRecoverListIndex, 63);
    l[63] = ~(uint64_t)0;
    fault("index 2^64 - 1", l, kRecoverListIndex, 63);
    l = range(0, 64);
    l[10] = 9;
    fault("a repeated index", l, kRecoverListOrder, 10);
    l = range(0, 64);
    l[10] = 11;
    l[11] = 10;
    fault("a descending pair", l, kRecoverListOrder, 11);
}

void empty_call() {
    RecoverSets s;
    const bool ok = recover_sets_of(s, nullptr, nullptr, 0) && s.sets.empty() && s.set_of.empty() && s.cell_off == std::vector<size_t>({0});
    report("n = 0", ok);
}

void single_list() {
    RecoverSet set;
    const std::vector<uint64_t> l = range(1, 128, 2);
    std::vector<uint64_t> exact(l);
    exact.shrink_to_fit();
    report("one list", recover_set_of(set, exact.data(), exact.size()) == kRecoverListGood && set_is(set, l));
}

// a shared-set call: one list for three blobs is one set, id 0 throughout and m cells per blob; a faulty list is reported as for one list
void shared_set() {
    const std::vector<uint64_t> l = range(1, 128, 2);
    std::vector<uint64_t> exact(l);
    exact.shrink_to_fit();
    const size_t m = l.size();
    RecoverSets s;
    bool ok = recover_sets_shared(s, exact.data(), m, 3) && s.fault == kRecoverListGood && s.sets.size() == 1 && set_is(s.sets[0], l);
    ok = ok && s.set_of == std::vector<uint32_t>({0, 0, 0}) && s.cell_off == std::vector<size_t>({0, m, 2 * m, 3 * m});
    std::string why;
    const auto faulty = [&](const char *name, const std::vector<uint64_t> &bad, RecoverListFault kind, size_t at) {
        std::vector<uint64_t> e(bad);
        e.shrink_to_fit();
        const bool same = !recover_sets_shared(s, e.data(), e.size(), 3) && s.fault == kind && (kind == kRecoverListCount || s.bad_at == at) &&
                          s.sets.empty();
        if (!same) why += std::string(" ") + name;
        ok = ok && same;
    };
    faulty("count 63", range(0, 63), kRecoverListCount, 0);
    faulty("count 129", range(0, 129), kRecoverListCount, 0);
    std::vector<uint64_t> b = range(0, 64);
    b[63] = 128;
    faulty("index 128", b, kRecoverListIndex, 63);
    b[63] = ~(uint64_t)0;
    faulty("index 2^64 - 1", b, kRecoverListIndex, 63);
    b = range(0, 64);
    b[10] = 9;
    faulty("a repeated index", b, kRecoverListOrder, 10);
    b = range(0, 64);
    b[10] = 11;
    b[11] = 10;
    faulty("a descending pair", b, kRecoverListOrder, 11);
    report("shared set, n = 3", ok, why);
}

}  // namespace

int main() {
    deduplication();
    offsets();
    faults();
    empty_call();
    single_list();
    shared_set();
    return failures;
}
