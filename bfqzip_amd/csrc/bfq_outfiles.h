// bfq_outfiles.h -- the output files of one *_fd call: committed at their final lengths, or left empty.  Host-only: no HIP
// types here.
// A member is the caller's descriptor (< 0: absent, skipped by everything below).  open() maps a regular file and pre-faults
// it in the background -- or picks up the mapping a tool registered with bfq_output_prefault() --; whatever cannot be mapped
// (a pipe, /dev/null, BFQ_NO_OUTMAP) is written through its descriptor.  at() is the destination bfq_write_async() and
// bfq_download() take.  commit() waits for the background writes and cuts every file to its length.  A set that goes
// uncommitted -- any exception on the way -- waits quietly, cuts every file to nothing, and takes a registered mapping of a
// member it never opened with it: "on failure they are left empty" needs no catch block.
// Declare the set AFTER every input mapping and every buffer the background writers read: it is then destroyed, and has
// waited for the writers, before they are released.
#pragma once
#include <errno.h>
#include <string.h>
#include <unistd.h>
#include <functional>
#include "bfq_internal_host.h"

// the final size of a file that was written through its descriptor (EINVAL: not a regular file, nothing to size);
// errnoText: strerror(errno) follows `what`
static inline void bfq_fd_size(int fd, u64 len, const char *what, bool errnoText = false)
{
    if (ftruncate(fd, (off_t)len) != 0 && errno != EINVAL) throw BfqError{BFQ_E_IO, errnoText ? std::string(what) + strerror(errno) : std::string(what)};
}

class OutFiles {
public:
    static const int MAX = 4;                                       // (the dedup: two kept texts, two removed)
    // drain(): every background write queued so far has arrived; it throws what went wrong
    OutFiles(const int *fd, int n, std::function<void()> drain) : n_(n < MAX ? n : MAX), drain_(std::move(drain))
    {
        for (int k = 0; k < n_; k++) of_[k].fd = fd[k];
    }
    OutFiles(int fd, std::function<void()> drain) : OutFiles(&fd, 1, std::move(drain)) {}
    OutFiles(const OutFiles &) = delete; OutFiles &operator=(const OutFiles &) = delete;
    ~OutFiles()
    {
        if (committed_) return;
        if (anyOpen_) { try { drain_(); } catch (...) {} }
        for (int k = 0; k < n_; k++) {
            Member &f = of_[k];
            if (f.fd < 0) continue;
            if (!f.opened) f.m = bfq_outmap_take(f.fd, 0);      // (a mapping the caller registered goes with the file's contents)
            close(f, 0);
        }
    }

    bool present(int k) const { return of_[k].fd >= 0; }
    void open(int k, u64 mapLen, u64 prefault)
    {
        Member &f = of_[k];
        if (f.fd < 0) return;
        f.m = bfq_outmap_take(f.fd, mapLen);
        if (f.m) bfq_outmap_extend(f.m, prefault);
        else f.m = bfq_outmap_open(f.fd, mapLen, prefault);
        f.opened = anyOpen_ = true;
    }
    // every member at its exact length: mapped with a page to spare, pre-faulted whole
    template <class L> void openAt(const L *len) { for (int k = 0; k < n_; k++) open(k, len[k] + 4096, len[k]); }
    HostRef at(int k, u64 off) const
    {
        const Member &f = of_[k];
        if (!f.m) return HostRef::file(f.fd, off);
        HostRef h = HostRef::mem(bfq_outmap_ptr(f.m) + off);
        h.om = f.m; h.off = off;
        return h;
    }
    // the text is known to reach `len`: more of the mapping is certain
    void extend(int k, u64 len)
    {
        bfq_outmap *m = of_[k].m;
        if (m && len > bfq_outmap_len(m)) throw BfqError{BFQ_E_IO, "output mapping smaller than the FASTQ text"};
        bfq_outmap_extend(m, len);
    }
    template <class L> void commit(const L *finalLen)                // (L: u64 or uint64_t, as the caller has them)
    {
        drain_();
        bool ok = true;
        for (int k = 0; k < n_; k++)
            if (of_[k].fd >= 0) ok = close(of_[k], finalLen[k]) && ok;
        if (!ok) throw BfqError{BFQ_E_IO, n_ == 1 ? "cannot size the output file" : "cannot size the output files"};
        committed_ = true;
    }

private:
    struct Member { int fd = -1; bfq_outmap *m = nullptr; bool opened = false; };
    static bool close(Member &f, u64 finalLen)
    {
        const bool ok = f.m ? bfq_outmap_close(f.m, finalLen) : ftruncate(f.fd, (off_t)finalLen) == 0 || errno == EINVAL;   // EINVAL: not a regular file
        f.m = nullptr;
        return ok;
    }
    Member of_[MAX];
    int n_;
    std::function<void()> drain_;
    bool anyOpen_ = false, committed_ = false;
};
