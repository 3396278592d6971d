// bfq_arena.h -- the device workspace as a value: a bump allocator over one buffer it does not own, and the guard that
// lends a context another buffer for a while.  Host-only: no HIP types here.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include "bfq_internal_host.h"

struct Arena {
    char *base = nullptr;
    size_t cap = 0, top = 0, peak = 0;
    void *alloc(size_t bytes)                                   // 256-byte aligned
    {
        const size_t a = (top + 255) & ~(size_t)255;
        if (a + bytes > cap) {
            char b[160];
            snprintf(b, sizeof b, "workspace exhausted: need %zu more bytes at %zu of %zu", bytes, a, cap);
            throw BfqError{BFQ_E_NOMEM, b};
        }
        top = a + bytes;
        if (top > peak) peak = top;
        return base + a;
    }
    size_t mark() const { return top; }
    void release(size_t m) { top = m; }
    size_t room() const { return cap - top; }
};

// Points c->ws at a foreign buffer; the previous arena comes back, `top` included, when the guard goes (or at restore()),
// after c->quiesce() has waited for the work that may still use the foreign one.  The high-water mark carries over.
// A context that has a poisonWs() is told of the new arena (bfq_ctx: the BFQ_POISON fill); one without it needs none.
template <class Ctx> static auto arena_lent(Ctx *c, int) -> decltype(c->poisonWs(), void()) { c->poisonWs(); }
template <class Ctx> static void arena_lent(Ctx *, long) {}
template <class Ctx> struct ScopedArenaT {
    Ctx *c;
    Arena prev;
    bool active = true;
    ScopedArenaT(Ctx *c, char *base, size_t cap) : c(c), prev(c->ws)
    {
        c->ws = Arena{base, cap, 0, prev.peak};
        try { arena_lent(c, 0); } catch (...) { c->ws = prev; throw; }   // BFQ_POISON: a lent buffer starts as dirty as the arena does
    }
    ScopedArenaT(const ScopedArenaT &) = delete; ScopedArenaT &operator=(const ScopedArenaT &) = delete;
    void restore()
    {
        if (!active) return;
        active = false;
        c->quiesce();
        prev.peak = c->ws.peak;
        c->ws = prev;
    }
    ~ScopedArenaT() { restore(); }
};
