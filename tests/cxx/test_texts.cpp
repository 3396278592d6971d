// test_texts.cpp -- bfq_texts.h on the host: the plan for the texts of a call against a table written out here, and the
// arena sizes of the line kernels against the allocations they stand for, made on an Arena over a malloc-ed buffer.
// Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_arena.h"
#include "../../bfqzip_amd/csrc/bfq_texts.h"

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); g_fail++; } } while (0)

static BfqTextSeen host_text(u64 len, u8 last)
{
    BfqTextSeen s;
    s.present = true; s.len = len; s.last = len ? last : 10;
    return s;
}
static BfqTextSeen dev_text(uintptr_t addr, u64 len, u8 last)
{
    BfqTextSeen s = host_text(len, last);
    s.device = true; s.addr = addr;
    return s;
}

struct PlanCase { const char *name; BfqTextSeen seen; bool addLf; bool present, moves; u64 len; };

static void plan_table()
{
    const uintptr_t A = 0x7f0000001000ull;                              // a multiple of 256
    const u8 LF = 10, G = 'G';
    const PlanCase T[] = {
        // a host text always moves; it gains its LF only when asked
        {"host lf", host_text(100, LF), false, true, true, 100},
        {"host lf +", host_text(100, LF), true, true, true, 100},
        {"host nolf", host_text(100, G), false, true, true, 100},
        {"host nolf +", host_text(100, G), true, true, true, 101},
        // a device text that ends in LF moves by its address alone
        {"dev+0 lf", dev_text(A + 0, 100, LF), false, true, false, 100},
        {"dev+1 lf", dev_text(A + 1, 100, LF), false, true, true, 100},
        {"dev+8 lf", dev_text(A + 8, 100, LF), false, true, true, 100},
        {"dev+16 lf", dev_text(A + 16, 100, LF), false, true, false, 100},
        {"dev+0 lf +", dev_text(A + 0, 100, LF), true, true, false, 100},
        {"dev+1 lf +", dev_text(A + 1, 100, LF), true, true, true, 100},
        {"dev+8 lf +", dev_text(A + 8, 100, LF), true, true, true, 100},
        {"dev+16 lf +", dev_text(A + 16, 100, LF), true, true, false, 100},
        // one that does not: as it is when no LF is added, moved and one byte longer when one is
        {"dev+0 nolf", dev_text(A + 0, 100, G), false, true, false, 100},
        {"dev+1 nolf", dev_text(A + 1, 100, G), false, true, true, 100},
        {"dev+8 nolf", dev_text(A + 8, 100, G), false, true, true, 100},
        {"dev+16 nolf", dev_text(A + 16, 100, G), false, true, false, 100},
        {"dev+0 nolf +", dev_text(A + 0, 100, G), true, true, true, 101},
        {"dev+1 nolf +", dev_text(A + 1, 100, G), true, true, true, 101},
        {"dev+8 nolf +", dev_text(A + 8, 100, G), true, true, true, 101},
        {"dev+16 nolf +", dev_text(A + 16, 100, G), true, true, true, 101},
        // present but empty: a slot all the same, and no LF to add; absent: nothing
        {"host empty", host_text(0, G), false, true, true, 0},
        {"host empty +", host_text(0, G), true, true, true, 0},
        {"dev empty", dev_text(A, 0, G), false, true, true, 0},
        {"dev empty +", dev_text(A, 0, G), true, true, true, 0},
        {"absent", BfqTextSeen{}, false, false, false, 0},
        {"absent +", BfqTextSeen{}, true, false, false, 0},
    };
    for (const PlanCase &c : T) {
        const BfqTextPlan P = bfq_texts_plan(&c.seen, 1, c.addLf);
        const BfqTextPlan::Slot &t = P.t[0];
        const bool ok = t.present == c.present && t.moves == c.moves && t.len == c.len && t.off == 0 &&
                        P.bufNeed == (c.moves ? ((size_t)c.len + 64 + 255) / 256 * 256 : 0) && !P.t[1].present && !P.t[2].present;
        if (!ok) { printf("FAIL plan case '%s'\n", c.name); g_fail++; }
    }
}

// three texts at once: the slots of those that move are 256-aligned, padded by 64 bytes at least, disjoint and in order, and
// bufNeed is the end of the last one
static void plan_three(const BfqTextSeen (&seen)[3], bool addLf, const bool (&moves)[3], const u64 (&len)[3])
{
    const BfqTextPlan P = bfq_texts_plan(seen, 3, addLf);
    size_t end = 0;
    for (int k = 0; k < 3; k++) {
        const BfqTextPlan::Slot &t = P.t[k];
        CHECK(t.present && t.moves == moves[k] && t.len == len[k]);
        if (!t.moves) continue;
        CHECK(t.off % 256 == 0 && t.off == end);
        end = t.off + ((size_t)t.len + 64 + 255) / 256 * 256;
        CHECK(end >= t.off + t.len + 64);
    }
    CHECK(P.bufNeed == end);
}

static std::string thrown_by(Arena &a, u64 len, u64 lines, bool index)
{
    try {
        bfq_nl_alloc(a, len);
        if (index) bfq_nl_alloc_ends(a, lines - 1);
    } catch (const BfqError &e) {
        return e.code == BFQ_E_NOMEM ? e.msg : "wrong code";
    }
    return "";
}

static void sizes()
{
    const u64 lens[] = {0, 1, 4095, 4096, 4097, (1ull << 20) + 1};
    for (u64 len : lens) {
        const u64 linesOf[] = {1, len + 1};
        for (u64 lines : linesOf) {
            for (int index = 0; index < 2; index++) {
                const size_t bytes = index ? bfq_line_index_bytes(len, lines) : bfq_count_lines_bytes(len);
                std::vector<char> buf(bytes + 256);
                char *base = (char *)(((uintptr_t)buf.data() + 255) & ~(uintptr_t)255);
                // the allocations fit into exactly what the size function says, from an aligned top and from an odd one
                Arena a{base, bytes, 0, 0};
                CHECK(thrown_by(a, len, lines, index).empty());
                const size_t used = a.top;
                CHECK(used <= bytes && used > 0);
                Arena odd{base, bytes, 1, 0};
                CHECK(thrown_by(odd, len, lines, index).empty());
                // ... and the function is tied to them: beyond what they used it counts the scan's partial sums and the
                // arena's alignment, nothing else
                CHECK(bytes <= used + bfq_scan_bytes((len + BFQ_NL_CHUNK - 1) / BFQ_NL_CHUNK) + 3 * 256);
                // an arena 256 bytes short of what they used is exhausted
                Arena shortBy{base, used - 256, 0, 0};
                CHECK(thrown_by(shortBy, len, lines, index).find("workspace exhausted") == 0);
            }
            // the record index on top of the line index: 44 bytes per record of four lines, the scan, the alignment
            const size_t N = (size_t)(lines / 4);
            const size_t rec = bfq_fastq_index_bytes(len, lines) - bfq_line_index_bytes(len, lines);
            CHECK(rec >= 32 * (N + 1) + 8 * (N + 2) + 4 * (N + 1) + bfq_scan_bytes(N) && rec <= 44 * (N + 2) + bfq_scan_bytes(N) + 3 * 256);
        }
    }
    // the scan: nothing up to one workgroup's items, two partial sums per workgroup above, level by level
    CHECK(bfq_scan_bytes(0) == 0 && bfq_scan_bytes(BFQ_SCAN_CHUNK) == 0);
    CHECK(bfq_scan_bytes(BFQ_SCAN_CHUNK + 1) == 2 * 256);
    CHECK(bfq_scan_bytes(100 * (u64)BFQ_SCAN_CHUNK) == 2 * 1024);
    CHECK(bfq_scan_bytes((u64)BFQ_SCAN_CHUNK * BFQ_SCAN_CHUNK + 1) == 2 * bfq_align256(8 * (BFQ_SCAN_CHUNK + 1)) + 2 * 256);
}

int main()
{
    plan_table();
    const uintptr_t A = 0x7f0000001000ull;
    {
        const BfqTextSeen s[3] = {host_text(4095, 'G'), dev_text(A, 4096, 10), dev_text(A + 8193, 4097, 10)};
        plan_three(s, true, {true, false, true}, {4096, 4096, 4097});
        plan_three(s, false, {true, false, true}, {4095, 4096, 4097});
    }
    {
        const BfqTextSeen s[3] = {host_text(1, 'G'), host_text(0, 'G'), dev_text(A + 16, 300, 'G')};
        plan_three(s, true, {true, true, true}, {2, 0, 301});
        plan_three(s, false, {true, true, false}, {1, 0, 300});
    }
    {   // an absent text between two present ones takes no room
        const BfqTextSeen s[3] = {host_text(500, 10), BfqTextSeen{}, host_text(700, 10)};
        const BfqTextPlan P = bfq_texts_plan(s, 3, true);
        CHECK(!P.t[1].present && !P.t[1].moves && P.t[1].len == 0);
        CHECK(P.t[0].off == 0 && P.t[2].off == 768 && P.bufNeed == 768 + 768);
    }
    sizes();
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("texts: all checks passed\n");
    return 0;
}
