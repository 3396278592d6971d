// bfq_internal_host.h -- host-only helpers of libbfqhip.so (bfq_host.cpp): no HIP types here.
#pragma once
#include <stdint.h>
#include <sys/mman.h>
#include <atomic>
#include <new>
#include <string>
#include "../../include/bfqzip_hip.h"
#include "bfq_common.h"

// what a failing stage throws: a BFQ_E_* code and the text bfq_last_error() returns
struct BfqError {
    int code;
    std::string msg;
};

// the body of a *_host entry point (no context): err, the calling thread's error string, is cleared first and receives what
// the body throws
template <class F> static int host_guarded(std::string &err, F body)
{
    err.clear();
    try {
        body();
        return BFQ_OK;
    } catch (const BfqError &e) {
        err = e.msg;
        return e.code;
    } catch (const std::bad_alloc &) {
        err = "host out of memory";
        return BFQ_E_NOMEM;
    }
}
static inline void zero3(uint64_t *a) { if (a) a[0] = a[1] = a[2] = 0; }

// an input file as read-only memory, unmapped when it goes.  open(): false with errno set; an empty file maps nothing.
struct MappedInput {
    void *p = MAP_FAILED; size_t n = 0;
    MappedInput() = default;
    MappedInput(const MappedInput &) = delete; MappedInput &operator=(const MappedInput &) = delete;
    bool open(int fd, size_t len) { n = len; p = len ? mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0) : MAP_FAILED; return !len || p != MAP_FAILED; }
    const uint8_t *data() const { return p != MAP_FAILED ? (const uint8_t *)p : nullptr; }
    ~MappedInput() { if (p != MAP_FAILED) munmap(p, n); }
};

// The BFQ_* environment variables.  bfq_env(): read once per process (first use) -- tracing, lease, thread counts.
// A context keeps its own copy, refreshed by bfq_create() and bfq_set_params() only (test knobs change between calls).
struct BfqEnv {
    bool trace = false;             // BFQ_TRACE: phase timeline, transfer rates, workspace allocations on stderr
    int piles = 0;                  // BFQ_PILES=1/0/2: step 1 pile by pile always / never, 2: the capped mode always (overrides bfq_params.piles); unset: 0
    bool pilesSplit = false;        // BFQ_PILES_SPLIT: every pile once more by its second symbol (test knob)
    bool noOverlap = false;         // BFQ_NO_OVERLAP: inversion and device -> host copies one after the other
    bool noLengthGuess = false;     // BFQ_NO_LENGTH_GUESS: always count read lengths by LF walks
    bool posMode = false;           // BFQ_POSMODE=1: steps 3-4 without LF table (position mode)
    bool posBins = true;            // BFQ_POSBINS=0: the device-resident fused path inverts by LF walks again (A/B runs)
    bool posBinWc = true;           // BFQ_POSBIN_WC=0: the position bins write per-tile runs at the bin's cursor again, not whole 64-byte chunks (A/B runs)
    bool posBinSparse = true;       // BFQ_POSBIN_SPARSE=0: every row travels through the position bins again, not only those that differ from the default (A/B runs)
    int posBinPolarity = -1;        // BFQ_POSBIN_POLARITY=keep|const: the sparse form's default is forced (const: M = 2 only); unset: chosen on the device
    bool fuseKeys = true;           // BFQ_FUSEKEYS=0: step 1 in one piece writes the sort records with k_build_keys and streams all five passes again (A/B runs)
    bool refinePipe = true;         // BFQ_REFINE_PIPE=0: the refinement's chunk kernel loads a round's third text word behind the first two again (k_refine_chunk_seq; A/B runs)
    int ioThreads = 0;              // BFQ_IO_THREADS: staging workers (0: by core count)
    int prefaultThreads = -1;       // BFQ_PREFAULT_THREADS: helpers that fault in output mappings (-1: by core count)
    unsigned long long hugeCap = 0; // BFQ_HUGE_CAP: slot budget of the huge-segment rounds (test knob)
    unsigned long long wsCap = 0;   // BFQ_WS_CAP: upper bound of the device workspace in bytes (suffixes K/M/G), 0: none
    int device = -1;                // BFQ_DEVICE: the GPU the one-shot tools use (-1: first free one, by lease)
    int fakeDevices = 0;            // BFQ_FAKE_DEVICES=n: pretend n GPUs (slot k -> device k mod the real count): lease tests on one GPU
    bool lease = true;              // BFQ_LEASE=0: no lease files (the caller places the tools itself)
    std::string leaseDir;           // BFQ_LEASE_DIR: where the lock files live (default /dev/shm, else /tmp)
    bool compact = false;           // BFQ_COMPACT=1: steps 2-4 on a given eBWT + LCP without the LF table whatever the cap (k_compact.hip; test knob)
    int dnaStatic = 0;              // BFQ_DNA_STATIC=1: read-order DNA through the static BFQRANS2 container as well (4x faster, 3x larger)
    int dnacK = 0, dnacH = 0, dnacW = 0, dnacSkip = -1;   // BFQ_DNAC_K / _H / _W / _TSKIP: the BFQDNAC1 container's parameters (the header carries them; defaults in k_dnac.hip)
    unsigned long long compactRing = 0; // BFQ_COMPACT_RING: entries of the interval refinement's ring queue there (default: what the cap leaves; small values test the chunked levels / the move to host memory)
    unsigned long long compactWin = 0;  // BFQ_COMPACT_WIN: rows of the LCP file in flight there (default 64 Mi; small values test the windowing)
    bool prefaultPause = false;     // BFQ_PREFAULT_PAUSE=1: output files are not allocated while an input file is being read (default: both at once)
    unsigned long long bgzfBatch = 0;   // BFQ_BGZF_BATCH: text bytes per batch of the BGZF writer (rounded down to whole members of 65 280; 0: chosen from the arena)
    int poison = -1;                // BFQ_POISON=<byte> (decimal or 0x.., 0-255): the arena is filled with it whenever a call starts over in it, every other
                                    // device allocation once when it is made (test knob: what a call must not read before it writes); unset: nothing is filled
    bool noOutmap = false;          // BFQ_NO_OUTMAP: the tools write their outputs with pwrite instead of through a mapping (test knob)
};
BfqEnv bfq_env_read();
const BfqEnv &bfq_env();
int bfq_cpu_budget();            // CPUs this process may keep busy (cgroup quota, affinity, hardware)
extern std::atomic<bool> g_bfqHipStarted;       // bfq_create() has initialised HIP: the output files' populate helpers may map pages now
extern std::atomic<int> g_bfqUploadsRunning;    // staged uploads in progress (bfq_io.hip): the output helpers stand back meanwhile

// output file mapped for writing, pre-faulted in the background
struct bfq_outmap;
bfq_outmap *bfq_outmap_open(int fd, uint64_t map_len, uint64_t prefault_len);
bfq_outmap *bfq_outmap_take(int fd, uint64_t min_len);     // a mapping registered by bfq_output_prefault(), or nullptr
char *bfq_outmap_ptr(bfq_outmap *m);
uint64_t bfq_outmap_len(bfq_outmap *m);
void bfq_outmap_extend(bfq_outmap *m, uint64_t prefault_len);
bool bfq_outmap_close(bfq_outmap *m, uint64_t final_len);
bool bfq_outmap_ensure(bfq_outmap *m, uint64_t off, uint64_t len);   // before copying into [off, off + len); false: use pwrite on bfq_outmap_fd()
int bfq_outmap_fd(bfq_outmap *m);

// a host-side operand of a transfer: memory, or an open file at an offset (the front-ends' files)
struct HostRef {
    void *ptr = nullptr; int fd = -1; u64 off = 0;
    bfq_outmap *om = nullptr;       // ptr lies `off` bytes into this output mapping: pages are populated before they are written
    static HostRef mem(const void *p) { HostRef h; h.ptr = const_cast<void *>(p); return h; }
    static HostRef file(int fd, u64 off = 0) { HostRef h; h.fd = fd; h.off = off; return h; }
    bool null() const { return !ptr && fd < 0; }
};
