// test_outfiles.cpp -- bfq_outfiles.h on the host: the output files of a call are committed at their lengths or left empty,
// whatever way the scope is left; registered mappings are picked up, replaced or taken along; pipes are written through their
// descriptor.  Built with the sanitizers over bfq_host.cpp: a mapping that is neither closed nor left registered is a leak.
// Files of a few KiB (no helper thread starts below 64 MiB); the drain is a counter that can be told to throw.
// Exit code 0 = all checks passed.
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <string>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_outfiles.h"

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); g_fail++; } } while (0)

static std::string g_dir;
static std::vector<std::string> g_paths;
static int tmp_file()
{
    const std::string p = g_dir + "/f" + std::to_string(g_paths.size());
    const int fd = open(p.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0600);
    if (fd < 0) { perror("open"); exit(2); }
    g_paths.push_back(p);
    return fd;
}
static long fsize(int fd)
{
    struct stat st;
    return fstat(fd, &st) == 0 ? (long)st.st_size : -1;
}
static std::string contents(int fd)
{
    std::string s((size_t)fsize(fd), '\0');
    CHECK(pread(fd, &s[0], s.size(), 0) == (ssize_t)s.size());
    return s;
}
static std::string pattern(size_t n, unsigned seed)
{
    std::string s(n, '\0');
    for (size_t i = 0; i < n; i++) s[i] = (char)('A' + (i * 7 + seed) % 23);
    return s;
}
// what the staging workers do with a destination (bfq_io.hip, host_put)
static void put(HostRef h, const std::string &s)
{
    if (h.ptr) {
        CHECK(bfq_outmap_ensure(h.om, h.off, s.size()));
        memcpy(h.ptr, s.data(), s.size());
    } else CHECK(pwrite(h.fd, s.data(), s.size(), (off_t)h.off) == (ssize_t)s.size());
}

// the drain: counts its calls, notes the size file `watch` had at the first one, throws when told to
struct Drain {
    int calls = 0, watch = -1;
    long sizeAtFirst = -1;
    bool fail = false;
    std::function<void()> fn()
    {
        return [this] {
            if (!calls++ && watch >= 0) sizeAtFirst = fsize(watch);
            if (fail) throw BfqError{BFQ_E_IO, "background write: told to fail"};
        };
    }
};

static const u64 LEN[2] = {5000, 3001};                                 // no multiples of the page size

static void commit_two()
{
    const int fd[2] = {tmp_file(), tmp_file()};
    const std::string want[2] = {pattern(LEN[0], 1), pattern(LEN[1], 2)};
    Drain d;
    d.watch = fd[0];
    {
        OutFiles F(fd, 2, d.fn());
        CHECK(fsize(fd[0]) == 0 && d.calls == 0);                       // construction touches nothing
        F.openAt(LEN);
        for (int k = 0; k < 2; k++) {
            CHECK(F.present(k) && F.at(k, 0).ptr != nullptr);
            CHECK(fsize(fd[k]) == (long)LEN[k] + 4096);
            put(F.at(k, 0), want[k]);
        }
        F.commit(LEN);
        CHECK(d.calls == 1 && d.sizeAtFirst == (long)LEN[0] + 4096);    // drained once, before the first close
    }
    CHECK(d.calls == 1);
    for (int k = 0; k < 2; k++) CHECK(fsize(fd[k]) == (long)LEN[k] && contents(fd[k]) == want[k]);
    close(fd[0]); close(fd[1]);
}

static void left_after_open()
{
    const int fd[2] = {tmp_file(), tmp_file()};
    Drain d;
    {
        OutFiles F(fd, 2, d.fn());
        F.openAt(LEN);
        put(F.at(0, 0), pattern(LEN[0], 3));
    }
    CHECK(d.calls == 1);
    CHECK(fsize(fd[0]) == 0 && fsize(fd[1]) == 0);
    close(fd[0]); close(fd[1]);
}

static void left_before_open_registered()
{
    const int fd[2] = {tmp_file(), tmp_file()};
    CHECK(bfq_output_prefault(fd[0], 8192, 4096) == BFQ_OK);
    CHECK(fsize(fd[0]) == 8192);
    Drain d;
    { OutFiles F(fd, 2, d.fn()); }
    CHECK(d.calls == 0);
    CHECK(fsize(fd[0]) == 0 && fsize(fd[1]) == 0);
    CHECK(bfq_outmap_take(fd[0], 0) == nullptr);                        // taken and closed, not left registered
    close(fd[0]); close(fd[1]);
}

static void registered_mappings()
{
    const std::string want = pattern(LEN[0], 4);
    {   // long enough: picked up
        const int fd = tmp_file();
        const u64 regLen = 3 * LEN[0] + 8192;
        CHECK(bfq_output_prefault(fd, regLen, 4096) == BFQ_OK);
        Drain d;
        OutFiles F(fd, d.fn());
        F.open(0, LEN[0] + 4096, LEN[0]);
        const HostRef h = F.at(0, 0);
        CHECK(h.om && bfq_outmap_len(h.om) == regLen && h.ptr == bfq_outmap_ptr(h.om));   // the registered mapping, not a new one
        CHECK(F.at(0, 100).ptr == bfq_outmap_ptr(h.om) + 100 && F.at(0, 100).off == 100);
        CHECK(bfq_outmap_take(fd, 0) == nullptr);
        put(h, want);
        F.commit(&LEN[0]);
        CHECK(fsize(fd) == (long)LEN[0] && contents(fd) == want);
        close(fd);
    }
    {   // too short: replaced
        const int fd = tmp_file();
        CHECK(bfq_output_prefault(fd, 4096, 4096) == BFQ_OK);
        Drain d;
        OutFiles F(fd, d.fn());
        F.open(0, LEN[0] + 4096, LEN[0]);
        const HostRef h = F.at(0, 0);
        CHECK(h.om && bfq_outmap_len(h.om) == LEN[0] + 4096);
        CHECK(bfq_outmap_take(fd, 0) == nullptr);
        put(h, want);
        F.commit(&LEN[0]);
        CHECK(fsize(fd) == (long)LEN[0] && contents(fd) == want);
        close(fd);
    }
}

static void absent_member()
{
    const int fd[3] = {tmp_file(), -1, tmp_file()};
    const u64 len[3] = {LEN[0], 12345, LEN[1]};
    const std::string want[3] = {pattern(len[0], 5), "", pattern(len[2], 6)};
    Drain d;
    {
        OutFiles F(fd, 3, d.fn());
        F.openAt(len);
        CHECK(F.present(0) && !F.present(1) && F.present(2));
        put(F.at(0, 0), want[0]); put(F.at(2, 0), want[2]);
        F.commit(len);
    }
    CHECK(contents(fd[0]) == want[0] && contents(fd[2]) == want[2]);
    { OutFiles F(fd, 3, d.fn()); F.open(1, 4096, 0); F.open(2, 4096, 0); }   // and by the destructor
    CHECK(fsize(fd[0]) == 0 && fsize(fd[2]) == 0);
    close(fd[0]); close(fd[2]);
}

static void pipe_member()
{
    int p[2];
    CHECK(pipe(p) == 0);
    const std::string want = pattern(700, 7);
    Drain d;
    {
        OutFiles F(p[1], d.fn());
        F.open(0, LEN[0] + 4096, LEN[0]);
        const HostRef h = F.at(0, 0);
        CHECK(h.ptr == nullptr && h.fd == p[1] && h.om == nullptr);
        F.extend(0, 1ull << 40);                                         // no mapping: nothing to outgrow
        CHECK(write(h.fd, want.data(), want.size()) == (ssize_t)want.size());
        const u64 n = want.size();
        F.commit(&n);                                                    // EINVAL from ftruncate is no failure
    }
    std::string got(want.size(), '\0');
    CHECK(read(p[0], &got[0], got.size()) == (ssize_t)got.size() && got == want);
    { OutFiles F(p[1], d.fn()); F.open(0, 4096, 0); }                    // nor for the destructor
    close(p[0]); close(p[1]);
}

static void extend_member()
{
    const int fd = tmp_file();
    Drain d;
    {
        OutFiles F(fd, d.fn());
        F.open(0, LEN[0] + 4096, 100);
        F.extend(0, LEN[0]);                                             // within the mapping: the pre-fault range grows
        F.extend(0, LEN[0] + 4096);
        int code = 0;
        std::string msg;
        try { F.extend(0, LEN[0] + 4097); }
        catch (const BfqError &e) { code = e.code; msg = e.msg; }
        CHECK(code == BFQ_E_IO && msg == "output mapping smaller than the FASTQ text");
        const std::string want = pattern(LEN[0], 8);
        put(F.at(0, 0), want);
        F.commit(&LEN[0]);
        CHECK(contents(fd) == want);
    }
    close(fd);
}

static void drain_throws()
{
    {   // inside commit: it propagates, the set stays uncommitted, the files end empty
        const int fd[2] = {tmp_file(), tmp_file()};
        Drain d;
        d.fail = true;
        int code = 0;
        std::string msg;
        try {
            OutFiles F(fd, 2, d.fn());
            F.openAt(LEN);
            put(F.at(1, 0), pattern(LEN[1], 9));
            F.commit(LEN);
            CHECK(!"commit returned");
        } catch (const BfqError &e) { code = e.code; msg = e.msg; }
        CHECK(code == BFQ_E_IO && msg == "background write: told to fail");
        CHECK(d.calls == 2);                                             // commit's, and the destructor's quiet one
        CHECK(fsize(fd[0]) == 0 && fsize(fd[1]) == 0);
        close(fd[0]); close(fd[1]);
    }
    {   // inside the destructor: swallowed
        const int fd[2] = {tmp_file(), tmp_file()};
        Drain d;
        d.fail = true;
        {
            OutFiles F(fd, 2, d.fn());
            F.openAt(LEN);
            put(F.at(0, 0), pattern(LEN[0], 10));
        }
        CHECK(d.calls == 1);
        CHECK(fsize(fd[0]) == 0 && fsize(fd[1]) == 0);
        close(fd[0]); close(fd[1]);
    }
}

static void fd_size()
{
    const int fd = tmp_file();
    bfq_fd_size(fd, 777, "cannot size the output file");
    CHECK(fsize(fd) == 777);
    close(fd);
    int p[2];
    CHECK(pipe(p) == 0);
    bfq_fd_size(p[1], 777, "cannot size the output file");              // not a regular file: tolerated
    close(p[0]); close(p[1]);
    std::string msg;
    try { bfq_fd_size(p[1], 1, "cannot size the output file: ", true); }   // a closed descriptor
    catch (const BfqError &e) { CHECK(e.code == BFQ_E_IO); msg = e.msg; }
    CHECK(msg == std::string("cannot size the output file: ") + strerror(EBADF));
}

int main()
{
    const char *base = getenv("TMPDIR");
    std::string tmpl = std::string(base && *base ? base : "/tmp") + "/bfq_outfiles_XXXXXX";
    if (!mkdtemp(&tmpl[0])) { perror("mkdtemp"); return 2; }
    g_dir = tmpl;
    commit_two();
    left_after_open();
    left_before_open_registered();
    registered_mappings();
    absent_member();
    pipe_member();
    extend_member();
    drain_throws();
    fd_size();
    for (const std::string &p : g_paths) unlink(p.c_str());
    rmdir(g_dir.c_str());
    if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
    printf("all checks passed\n");
    return 0;
}
