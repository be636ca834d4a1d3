// lds_pad_check.cpp -- the decision of lambdaworks_kzg_amd/csrc/lds_pad.h on the host, built with -fsanitize=address,undefined
// (tests/test_lds_pad_cpu.py). A fake runtime stands where HIP would: it answers the two LDS queries, records the dynamic-LDS value of
// every launch and refuses what it is told to refuse; its error state reads like HIP's (peek leaves it, take clears it). Prints one line
// per case, "name: the launches' LDS values | pending error afterwards | refused latch", which the Python side compares; exit status 1
// if a case could not even be set up.
#include <stdio.h>

#include <string>
#include <vector>

#include "lds_pad.h"

namespace {

constexpr uint32_t KiB = 1024u, kLimit = 160 * KiB, kDecompressStatic = 56 * KiB;

struct FakeRt {
    uint32_t stat, limit;
    int refuse_pad = 0, refuse_plain = 0, refuse_raise = 0;   // the error a launch with a pad / without one / the attribute returns (0: accepted)
    int pending = 0;
    std::vector<uint32_t> calls, raises;
    int queries = 0;
    uint32_t lds_static() { queries++; return stat; }
    uint32_t lds_limit() { queries++; return limit; }
    int raise(uint32_t bytes) {
        raises.push_back(bytes);
        if (refuse_raise) pending = refuse_raise;
        return refuse_raise;
    }
    int peek() const { return pending; }
    int take() {
        const int e = pending;
        pending = 0;
        return e;
    }
    void launch(uint32_t lds) {
        calls.push_back(lds);
        if (const int e = lds ? refuse_pad : refuse_plain) pending = e;
    }
};

void report(const char *name, FakeRt &rt, const lwk::PadCache &c, int dev) {
    std::string s;
    for (uint32_t v : rt.calls) s += (s.empty() ? "" : ",") + std::to_string(v);
    printf("%s: %s | pending %d | refused %d | queries %d\n", name, s.c_str(), rt.pending, (int)c.dev[dev].refused.load(), rt.queries);
    rt.calls.clear();
    rt.queries = 0;
}

}  // namespace

int main() {
    {   // 1. pads that fit pass unchanged, in one launch; the queries are made once per (kernel, device)
        lwk::PadCache k_dec, k_sub;
        FakeRt dec{kDecompressStatic, kLimit}, sub{0, kLimit};
        lwk::launch_padded(k_dec, 0, 60 * KiB, dec);
        report("fit 56+60", dec, k_dec, 0);
        lwk::launch_padded(k_dec, 0, 60 * KiB, dec);
        report("fit 56+60 again", dec, k_dec, 0);
        lwk::launch_padded(k_sub, 0, 116 * KiB, sub);
        report("fit 0+116", sub, k_sub, 0);
        lwk::launch_padded(k_sub, 0, 0, sub);
        report("no pad wanted", sub, k_sub, 0);
        if (dec.raises != std::vector<uint32_t>{60 * KiB} || sub.raises != std::vector<uint32_t>{116 * KiB}) return 1;   // the attribute: once each
    }
    {   // 2. the clamp
        lwk::PadCache a, b, c;
        FakeRt dec{kDecompressStatic, kLimit}, sub{0, kLimit}, big{kLimit + 4096, kLimit};
        lwk::launch_padded(a, 0, 150 * KiB, dec);
        report("clamp 56+150", dec, a, 0);
        lwk::launch_padded(b, 0, 150 * KiB, sub);
        report("clamp 0+150", sub, b, 0);
        lwk::launch_padded(c, 0, 60 * KiB, big);
        report("static above limit", big, c, 0);
    }
    {   // 3. a runtime that refuses any pad: two launches the first time, one from then on; other kernels and devices are not latched
        lwk::PadCache k, other;
        FakeRt rt{0, kLimit};
        rt.refuse_pad = 701;
        lwk::launch_padded(k, 3, 116 * KiB, rt);
        report("refused first", rt, k, 3);
        lwk::launch_padded(k, 3, 116 * KiB, rt);
        report("refused later", rt, k, 3);
        rt.refuse_pad = 0;
        lwk::launch_padded(k, 4, 116 * KiB, rt);
        report("other device", rt, k, 4);
        lwk::launch_padded(other, 3, 116 * KiB, rt);
        report("other kernel", rt, other, 3);
        lwk::launch_padded(k, lwk::kPadMaxDevices, 116 * KiB, rt);
        report("ordinal beyond the table", rt, k, 0);
    }
    {   // 4. everything refused: two launches, the second one's error is left standing
        lwk::PadCache k;
        FakeRt rt{0, kLimit};
        rt.refuse_pad = 701, rt.refuse_plain = 98;
        lwk::launch_padded(k, 0, 116 * KiB, rt);
        report("both refused", rt, k, 0);
    }
    {   // 5. an error already pending: one plain launch, the error still there, nothing latched
        lwk::PadCache k;
        FakeRt rt{0, kLimit};
        rt.pending = 719;
        lwk::launch_padded(k, 0, 116 * KiB, rt);
        report("pending", rt, k, 0);
    }
    {   // the attribute refused: no padded launch at all, the plain one, latched
        lwk::PadCache k;
        FakeRt rt{0, kLimit};
        rt.refuse_raise = 1;
        lwk::launch_padded(k, 0, 116 * KiB, rt);
        report("attribute refused", rt, k, 0);
    }
    return 0;
}
