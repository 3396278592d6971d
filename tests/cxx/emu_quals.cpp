// emu_quals.cpp -- the kernels of bfqzip_amd/csrc/k_quals.hip run on the CPU, one thread, as a program of its own under
// -fsanitize=address,undefined: k_ql_count, k_ql_encode and k_ql_decode against a container made by tests/quals_model.py.
// tests/test_quals_host.py cuts the kernels out of k_quals.hip (from "#define QL_S" to the host side) into
// k_quals_kernels.inc and compiles this file beside it; the few HIP words the kernels use are defined below.
//   emu_quals DIR    DIR/in.bin the stream, DIR/cont.bin its container, DIR/cnt.bin the counts at the container's rung (u32)
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <string>
typedef uint8_t u8; typedef uint16_t u16; typedef uint32_t u32; typedef uint64_t u64;
#define __global__
#define __device__
#define __host__
#define __shared__ static
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#pragma GCC diagnostic ignored "-Wunknown-pragmas"
struct D3 { unsigned x, y, z; };
static D3 threadIdx{0, 0, 0}, blockIdx{0, 0, 0}, blockDim{1, 1, 1}, gridDim{1, 1, 1};
static void __syncthreads() {}
static u32 atomicAdd(u32 *p, u32 v) { u32 o = *p; *p += v; return o; }
static u32 atomicCAS(u32 *p, u32 c, u32 v) { u32 o = *p; if (o == c) *p = v; return o; }
static u32 atomicMax(u32 *p, u32 v) { u32 o = *p; if (v > o) *p = v; return o; }
struct uint4 { u32 x, y, z, w; };
static u32 bfq_lane() { return 0; }
#include "k_quals_kernels.inc"
static std::vector<u8> rd(const std::string &p) { FILE *f = fopen(p.c_str(), "rb"); if (!f) { perror(p.c_str()); exit(2); } std::vector<u8> v; u8 b[65536]; size_t n; while ((n = fread(b, 1, sizeof b, f)) > 0) v.insert(v.end(), b, b + n); fclose(f); return v; }
int main(int argc, char **argv)
{
    const std::string d = argv[1];
    // exact-size heap copies so that the sanitizer sees every byte past the end
    std::vector<u8> in0 = rd(d + "/in.bin"), ct = rd(d + "/cont.bin"), cn = rd(d + "/cnt.bin");
    const u64 n = in0.size();
    u8 *in = (u8 *)malloc(n); memcpy(in, in0.data(), n);
    const u8 *h = ct.data();
    const u64 nreads = ql_get64(h + 16), nvals = ql_get64(h + 24), ll = ql_get64(h + 64);
    const u32 nseg = ql_get32(h + 36), A = ql_get32(h + 40), rung = ql_get32(h + 44), maxlen = ql_get32(h + 52);
    const u64 rows = ql_rows(rung, A);
    const u8 *alpha = h + QL_HDR + ll, *dfl = alpha + 64, *used = dfl + 2 * A, *rp = used + (rows + 7) / 8;
    std::vector<u32> lens(nreads); std::vector<u64> boff(nreads + 1);
    { u64 r = 0, st = 0, o = 0; for (u64 i = 0; i < n; i++) if (in[i] == 10) { lens[r] = (u32)(i - st); boff[r] = o; o += i - st; r++; st = i + 1; } boff[nreads] = o; if (o != nvals || r != nreads) { printf("bad split\n"); return 1; } }
    u64 *segFirst = (u64 *)malloc(8 * (nseg + 1));
    k_ql_segfirst(boff.data(), nreads, nseg, segFirst);
    u8 map[256] = {0};
    for (u32 s = 0; s < A; s++) map[alpha[s]] = (u8)s;
    QlIn I{in, n, boff.data(), segFirst, nseg};
    const QlPar P = ql_par(A, rung, maxlen);
    // count
    u32 *cnt = (u32 *)calloc(rows * A, 4);
    k_ql_count(I, map, P, 1, cnt);
    if (cn.size() != rows * A * 4 || memcmp(cn.data(), cnt, cn.size())) { printf("COUNT DIFFERS\n"); return 1; }
    // model tables
    std::vector<u32> fc(rows * A);
    const u32 nld = (A + 7) / 8, Ap = 8 * nld;
    u16 *cum = (u16 *)malloc(2 * rows * Ap);
    for (u64 x = 0; x < rows; x++) {
        const u8 *row = dfl;
        if ((used[x >> 3] >> (x & 7)) & 1) { row = rp; rp += 2 * A; }
        u32 acc = 0;
        for (u32 s = 0; s < Ap; s++) {
            cum[x * Ap + s] = (u16)(s < A ? acc : 4096);
            if (s < A) { const u32 f = row[2 * s] | (row[2 * s + 1] << 8); fc[x * A + s] = f | (acc << 16); acc += f; }
        }
    }
    const u8 *segtab = rp, *pay = rp + 4 * (u64)nseg;
    // encode
    const u64 ssz = 2 * nvals + 16 * ((u64)nseg + 1);
    u8 *scratch = (u8 *)malloc(ssz);
    u32 *segBytes = (u32 *)malloc(4 * (u64)nseg);
    k_ql_encode(I, map, P, fc.data(), scratch, segBytes);
    u64 o = 0;
    for (u32 g = 0; g < nseg; g++) {
        if (segBytes[g] != ql_get32(segtab + 4 * (u64)g)) { printf("SEG BYTES DIFFER at %u: %u vs %u\n", g, segBytes[g], ql_get32(segtab + 4 * (u64)g)); return 1; }
        const u8 *src = scratch + ql_slot_end(boff[segFirst[g + 1]], g) - segBytes[g];
        if (memcmp(src, pay + o, segBytes[g])) { printf("PAYLOAD DIFFERS in segment %u\n", g); return 1; }
        o += segBytes[g];
    }
    if ((u64)(pay - h) + o != ct.size()) { printf("LENGTH DIFFERS\n"); return 1; }
    // decode (from an exact-size copy of the payload)
    u8 *pc = (u8 *)malloc(o ? o : 1); memcpy(pc, pay, o);
    std::vector<u64> off(nseg + 1, 0);
    for (u32 g = 0; g < nseg; g++) off[g + 1] = off[g] + segBytes[g];
    u8 *out = (u8 *)malloc(n);
    memset(out, 0, n);
    u32 bad = 0;
    QlIn J{nullptr, n, boff.data(), segFirst, nseg};
    k_ql_decode(J, pc, off.data(), segBytes, alpha, P, cum, nld, out, &bad);
    k_ql_newlines(boff.data(), nreads, out);
    if (bad || memcmp(out, in, n)) { printf("DECODE DIFFERS (bad %u)\n", bad); return 1; }
    // a damaged payload: some 150 bytes flipped in turn -- the decoder must stay inside (the sanitizer watches)
    if (o < 100000) for (u64 k = 0; k < o; k += o / 150 + 1) { pc[k] ^= 0x55; bad = 0; k_ql_decode(J, pc, off.data(), segBytes, alpha, P, cum, nld, out, &bad); pc[k] ^= 0x55; }
    printf("ok %s rung %u A %u nseg %u\n", d.c_str(), rung, A, nseg);
    return 0;
}
