// pre_cadence_check.cpp — a stand-alone host program over pre_cadence_ok (nns_internal.h), the closed form behind the
// int8 pre-pass's barrier cadence (OpI8Pre, filter_mfma.hip: one workgroup barrier per G intervals).  No device is
// touched.  Build (host pass only):
//   hipcc --offload-arch=gfx950 --cuda-host-only -std=c++17 -Iinclude -Inns-cuda_amd/csrc tools/pre_cadence_check.cpp -o pre_cadence_check
// The protocol, as the kernel runs it on a ring of D slots with a DMA lead of A intervals:
//   prologue   issue slots 0 .. A-1; wait until at most N0 of the wave's slots are in flight (G = 1: N0 = A - 1, else
//              N0 = A - G - 1); barrier; read slot 0 (first fragments, first seeds)
//   interval s if s % G == 0: wait until at most N = A - G - 1 slots are in flight, barrier;
//              then read slots s and s + 1 (the last fragments' prefetch and the next tile's seeds; nothing of slot ns)
//              and issue slot s + A
// A wave's DMA into a slot may land at any time between its issue and the wave's own counted wait that confirms it; a
// slot is readable once every wave has confirmed its share and a barrier has passed.  Between two barriers every wave is
// somewhere inside the same group of intervals, and that is all the barriers say.  For every pair of positions they allow
// the program checks that
//   * no slot a wave reads is unconfirmed, and
//   * no slot that a wave may still be writing shares a ring position with a slot another wave (or itself) reads,
// and that pre_cadence_ok accepts exactly the (A, G) for which both hold on every stream length tried.
// The closed form rests on an interval reading slots s and s + 1 only: the pre-pass refinement takes nothing from the ring.
// The model has a switch for the other case (reads_prev: interval s also re-reads slot s - 1, as lazy16's refinement
// does); there the safe set is G < A && A + G < D — one less — and the program checks that too, so that what a ring
// re-read would cost is on record: AHEAD + G == depth (12 with 4) is accepted today and would not be then.
#include <stdio.h>
#include <algorithm>
#include "nns_internal.h"

// the kernel's counted waits, in slots (a negative count cannot be written: the wait then leaves nothing in flight)
static int wait_prologue(int A, int G) { return std::max(0, G == 1 ? A - 1 : A - G - 1); }
static int wait_loop(int A, int G) { return std::max(0, A - G - 1); }

// one stream of ns slots; returns the number of violations (why: the first one, for the report)
static int brute(int D, int A, int G, int ns, bool reads_prev, char *why, size_t nwhy)
{
    int bad = 0;
    auto fail = [&](const char *what, int g, int sa, int sb, int slot) {
        if (!bad) snprintf(why, nwhy, "%s: D %d A %d G %d ns %d group %d, intervals %d / %d, slot %d", what, D, A, G, ns, g, sa, sb, slot);
        ++bad;
    };
    // prologue segment: every wave has issued 0 .. A-1 and reads slot 0
    int confirmed = A - 1 - wait_prologue(A, G);
    if (confirmed < 0) fail("read of an unconfirmed slot (prologue)", -1, 0, 0, 0);
    for (int t = confirmed + 1; t <= A - 1; ++t)
        if (t % D == 0) fail("write into a readable slot (prologue)", -1, 0, 0, t);
    for (int g = 0; g * G < ns; ++g) {
        const int s0 = g * G, s1 = std::min(s0 + G, ns);   // the group's intervals
        // every wave ran the barrier's wait with slots .. s0 - 1 + A issued
        confirmed = std::max(confirmed, s0 - 1 + A - wait_loop(A, G));
        for (int sa = s0; sa < s1; ++sa)            // the writer: anything up to sa + A may be issued, nothing newer confirmed
            for (int sb = s0; sb < s1; ++sb) {      // the reader
                const int reads[3] = {sb, sb + 1 < ns ? sb + 1 : sb, reads_prev && sb > 0 ? sb - 1 : sb};
                for (int r : reads) {
                    if (r > confirmed) fail("read of an unconfirmed slot", g, sa, sb, r);
                    for (int t = confirmed + 1; t <= sa + A; ++t)
                        if (t != r && (t - r) % D == 0) fail("write into a readable slot", g, sa, sb, t);
                }
            }
    }
    return bad;
}

int main()
{
    constexpr int D = nns::kI8PreRingDepth;
    static_assert(D == 16, "the check's table is for the ring of sixteen");
    int wrong = 0, accepted = 0;
    char why[256];
    for (int A = 2; A <= D - 1; ++A)
        for (int G = 1; G <= 8; ++G) {
            int bad = 0, bad_prev = 0;
            why[0] = 0;
            // stream lengths: shorter than a group, partial last groups, several ring turns
            for (int ns = 1; ns <= 4 * D + 2 * G + 1; ++ns) {
                char w[256] = "";
                const int b = brute(D, A, G, ns, false, w, sizeof w);
                if (b && !bad) snprintf(why, sizeof why, "%s", w);
                bad += b;
                bad_prev += brute(D, A, G, ns, true, w, sizeof w);
            }
            // (a refinement that re-read slot s - 1: one slot less)
            if ((G < A && A + G < D) != (bad_prev == 0)) {
                printf("reads_prev: A + G < D %s but the protocol is %s: A %d G %d\n", (G < A && A + G < D) ? "holds" : "fails",
                       bad_prev ? "unsafe" : "safe", A, G);
                ++wrong;
            }
            const bool ok = nns::pre_cadence_ok(D, A, G);
            accepted += ok;
            if (ok != (bad == 0)) {
                printf("closed form %s but the protocol is %s: A %d G %d%s%s\n", ok ? "accepts" : "rejects", bad ? "unsafe" : "safe", A, G,
                       bad ? " — " : "", why);
                ++wrong;
            }
        }
    // the product's own constants
    char w[256] = "";
    int pbad = 0;
    for (int ns = 1; ns <= 4 * D + 2 * nns::kI8PreGroup + 1; ++ns) pbad += brute(D, nns::kI8PreAhead, nns::kI8PreGroup, ns, false, w, sizeof w);
    if (!nns::pre_cadence_ok(D, nns::kI8PreAhead, nns::kI8PreGroup) || pbad) {
        printf("the build's cadence is unsafe: AHEAD %d G %d %s\n", nns::kI8PreAhead, nns::kI8PreGroup, w);
        ++wrong;
    }
    if (wrong) return 1;
    printf("pre cadence ok: ring %d, AHEAD 2 .. %d x G 1 .. 8, %d combinations accepted, all and only the safe ones; build AHEAD %d G %d\n", D,
           D - 1, accepted, nns::kI8PreAhead, nns::kI8PreGroup);
    return 0;
}
