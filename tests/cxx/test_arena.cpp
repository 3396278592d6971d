// test_arena.cpp -- bfq_arena.h on the host: the bump allocator over a malloc-ed buffer, and ScopedArenaT with a context
// whose quiesce() only counts.  Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../bfqzip_amd/csrc/bfq_arena.h"

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); g_fail++; } } while (0)

struct FakeCtx {
    Arena ws;
    int syncs = 0, fills = 0;
    void quiesce() { syncs++; }
    void poisonWs() { fills++; }                                       // told of every buffer that is lent as the arena
};
struct BareCtx {
    Arena ws;
    int syncs = 0;
    void quiesce() { syncs++; }
};
static bool same(const Arena &a, const Arena &b) { return a.base == b.base && a.cap == b.cap && a.top == b.top; }

int main()
{
    const size_t CAP = 1 << 16;
    char *buf = (char *)aligned_alloc(256, CAP), *other = (char *)aligned_alloc(256, 4096);
    Arena a{buf, CAP, 0, 0};

    // alignment, bounds and the high-water mark over odd sizes
    size_t peak = 0;
    const size_t sizes[] = {1, 255, 256, 257, 0, 1000, 4095, 3};
    for (size_t s : sizes) {
        const size_t before = a.top;
        char *p = (char *)a.alloc(s);
        CHECK(((uintptr_t)p & 255) == 0);
        CHECK(p >= buf + before && p + s <= buf + CAP);
        CHECK(a.top == (size_t)(p - buf) + s);
        CHECK(a.peak >= peak && a.peak >= a.top);
        peak = a.peak;
        CHECK(a.room() == CAP - a.top);
    }

    // mark / release nest; the peak never comes down
    const size_t m1 = a.mark();
    a.alloc(500);
    const size_t m2 = a.mark();
    a.alloc(9000);
    CHECK(a.mark() > m2 && m2 > m1);
    const size_t high = a.peak;
    a.release(m2);
    CHECK(a.mark() == m2 && a.room() == CAP - m2);
    char *again = (char *)a.alloc(10);
    CHECK((size_t)(again - buf) == ((m2 + 255) & ~(size_t)255));      // the released space is handed out again
    a.release(m1);
    CHECK(a.mark() == m1 && a.peak == high);

    // what does not fit throws BFQ_E_NOMEM and leaves the arena as it was
    for (size_t want : {a.room() + 1, CAP, (size_t)-1 / 2}) {
        const Arena before = a;
        bool thrown = false;
        try { a.alloc(want); } catch (const BfqError &e) { thrown = e.code == BFQ_E_NOMEM && e.msg.find("workspace exhausted") == 0; }
        CHECK(thrown && same(a, before) && a.peak == before.peak);
    }
    a.release((a.top + 255) & ~(size_t)255);
    CHECK(a.alloc(a.room()) != nullptr && a.room() == 0);             // exactly what is left still fits
    a.release(m1);

    // ScopedArenaT: the context's arena comes back with base, cap and top -- at the end of the scope,
    FakeCtx c;
    c.ws = a;
    const Arena own = c.ws;
    {
        ScopedArenaT<FakeCtx> g(&c, other, 4096);
        CHECK(c.ws.base == other && c.ws.cap == 4096 && c.ws.top == 0);
        CHECK((char *)c.ws.alloc(100) == other);
        CHECK(c.syncs == 0 && c.fills == 1);
    }
    CHECK(same(c.ws, own) && c.syncs == 1 && c.fills == 1);             // ... and not of the one that comes back
    // ... at an early restore(), once,
    {
        ScopedArenaT<FakeCtx> g(&c, other, 4096);
        c.ws.alloc(300);
        g.restore();
        CHECK(same(c.ws, own) && c.syncs == 2);
        c.ws.alloc(64);                                                // the context's own arena is in use again
        g.restore();
    }
    CHECK(c.syncs == 2 && c.ws.base == buf && c.ws.top > own.top);
    c.ws.release(own.top);
    // ... and while a throw unwinds, before the handler runs
    bool seen = false;
    try {
        ScopedArenaT<FakeCtx> g(&c, other, 4096);
        c.ws.alloc(4000);
        c.ws.alloc(4000);                                              // throws: 4096 bytes
        CHECK(!"not reached");
    } catch (const BfqError &e) {
        seen = e.code == BFQ_E_NOMEM && same(c.ws, own) && c.syncs == 3;
    }
    CHECK(seen && c.fills == 3);
    CHECK(c.ws.peak >= own.peak);                                      // the high-water mark carries over
    // a context without poisonWs() is lent a buffer all the same
    BareCtx bare;
    bare.ws = a;
    {
        ScopedArenaT<BareCtx> g(&bare, other, 4096);
        CHECK(bare.ws.base == other && (char *)bare.ws.alloc(100) == other && bare.syncs == 0);
    }
    CHECK(same(bare.ws, a) && bare.syncs == 1);

    free(buf); free(other);
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("arena: all checks passed\n");
    return 0;
}
