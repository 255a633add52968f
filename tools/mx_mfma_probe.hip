// mx_mfma_probe.hip -- what v_mfma_scale_f32_16x16x128_f8f6f4 does BY ITSELF with the bytes of the packed MX export (DESIGN.md
// section 9.14): one instruction per case on hand-built operands, no part of ppq_amd involved.  ppq_amd/csrc/mx_gemm.hip decides NaN
// itself, so its tests cannot show the instruction's own behaviour; this prints it.
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/mx_mfma_probe.hip -o mx_mfma_probe && ./mx_mfma_probe
//
// Cases, per line one verdict:
//   order    for each of the five formats as A against E4M3 as B (and the other way round): element i of the dense little-endian
//            bit string of lane (row r, K-group g) meets byte i of the E4M3 lane of the same K-group and no other.  FP8 against FP8
//            says yes under any map both sides share; FP6 / FP4 say NO because an FP8 lane's bytes are not one block (see kmap)
//   kmap     which k every (K-group, element) of an operand is, and whose scale it takes, in the frame of an FP4 operand
//   kgroup   lane l >> 4 is the K-group: a 1.0 in group g of A meets only group g of B
//   opsel    which byte of the scale register opsel 0 .. 3 selects, for A and for B
//   scale    a scale code per lane is applied to that lane's block only; codes 0 and 254
//   nan      scale 0xFF, the FP8 NaN codes and the E5M2 Inf codes: what comes out, and where
//   width    2^e - 2^e + 1 and 2^e + 1 inside one instruction, the 1 in another block, for growing e: what the internal sum keeps
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

struct Operands {
    uint32_t a[64][8], b[64][8];                  // the lanes' operand registers
    uint32_t sa[64], sb[64];                      // the lanes' scale registers
};

template <int CBSZ, int BLGP, int OPA, int OPB>
__global__ void probe_kernel(const Operands* in, float* out) {
    const int l = threadIdx.x;
    v8i a, b;
    for (int w = 0; w < 8; w++) { a[w] = (int)in->a[l][w]; b[w] = (int)in->b[l][w]; }
    v4f c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, CBSZ, BLGP, OPA, (int)in->sa[l], OPB, (int)in->sb[l]);
    for (int q = 0; q < 4; q++) out[(4 * (l >> 4) + q) * 16 + (l & 15)] = c[q];          // row-major [16][16]
}

// the instruction's format ids
enum { E4M3 = 0, E5M2 = 1, E2M3 = 2, E3M2 = 3, E2M1 = 4 };
static const char* kNames[5] = {"E4M3", "E5M2", "E2M3", "E3M2", "E2M1"};
static const int kBits[5] = {8, 8, 6, 6, 4};
static const uint32_t kOne[5] = {0x38, 0x3c, 0x08, 0x0c, 0x02};                          // the code of 1.0

static Operands* d_in;
static float* d_out;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

template <int CBSZ, int BLGP, int OPA, int OPB>
static void run_t(const Operands& op, float (&c)[16][16]) {
    CHECK(hipMemcpy(d_in, &op, sizeof(op), hipMemcpyHostToDevice));
    hipLaunchKernelGGL((probe_kernel<CBSZ, BLGP, OPA, OPB>), dim3(1), dim3(64), 0, 0, d_in, d_out);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(&c[0][0], d_out, sizeof(c), hipMemcpyDeviceToHost));
}
template <int CBSZ>
static void run_b(int blgp, const Operands& op, float (&c)[16][16]) {
    switch (blgp) {
        case 0: run_t<CBSZ, 0, 0, 0>(op, c); break;
        case 1: run_t<CBSZ, 1, 0, 0>(op, c); break;
        case 2: run_t<CBSZ, 2, 0, 0>(op, c); break;
        case 3: run_t<CBSZ, 3, 0, 0>(op, c); break;
        default: run_t<CBSZ, 4, 0, 0>(op, c); break;
    }
}
static void run(int cbsz, int blgp, const Operands& op, float (&c)[16][16]) {
    switch (cbsz) {
        case 0: run_b<0>(blgp, op, c); break;
        case 1: run_b<1>(blgp, op, c); break;
        case 2: run_b<2>(blgp, op, c); break;
        case 3: run_b<3>(blgp, op, c); break;
        default: run_b<4>(blgp, op, c); break;
    }
}

// element i of a lane's dense little-endian bit string
static void put(uint32_t (&reg)[8], int bits, int i, uint32_t code) {
    const int at = i * bits, w = at >> 5, off = at & 31;
    reg[w] |= code << off;
    if (off + bits > 32) reg[w + 1] |= code >> (32 - off);
}
static void clear(Operands& op) {
    memset(&op, 0, sizeof(op));
    for (int l = 0; l < 64; l++) { op.sa[l] = 127; op.sb[l] = 127; }
}
static void fill(uint32_t (&reg)[8], int fmt, uint32_t code) {
    for (int i = 0; i < 32; i++) put(reg, kBits[fmt], i, code);
}
static uint32_t bits_of(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

static void probe_order() {
    // lane (r, g) of the tested operand holds 1.0 at element (8 g + r + 16 h) % 32 ...; the E4M3 lane (c, g) holds 1.0 at byte
    // (8 g + c + 16 h) % 32: C[r][c] = number of g with equal positions = 4 [r == c]
    for (int side = 0; side < 2; side++) {
        for (int fmt = 0; fmt < 5; fmt++) {
            bool ok = true;
            for (int h = 0; h < 2; h++) {
                Operands op; clear(op);
                for (int l = 0; l < 64; l++) {
                    const int r = l & 15, g = l >> 4, pos = (8 * g + r + 16 * h) % 32;
                    put(side == 0 ? op.a[l] : op.b[l], kBits[fmt], pos, kOne[fmt]);
                    put(side == 0 ? op.b[l] : op.a[l], 8, pos, kOne[E4M3]);
                }
                float c[16][16];
                run(side == 0 ? fmt : E4M3, side == 0 ? E4M3 : fmt, op, c);
                for (int r = 0; r < 16; r++)
                    for (int q = 0; q < 16; q++) ok = ok && c[r][q] == (r == q ? 4.f : 0.f);
            }
            printf("order   %s as %c against E4M3 bytes: dense little-endian element i meets byte i: %s\n", kNames[fmt], side == 0 ? 'A' : 'B', ok ? "yes" : "NO");
        }
    }
}

// Where element p of lane (row, K-group g) sits along K, and whose scale it takes, for every format on either side.  The frame is
// FP4 on the other side, taken as k = 32 g' + p' under the scale of lane g' (probe_scale shows that an FP4 lane's scale covers its
// own 32 elements).  The tested operand holds one 1.0 per row, at (g, p), under scale codes 127 + 4 g'' per K-group g''; column c of
// the FP4 operand holds 1.0 at p' = c and 3.0 at p' = c + 16 in every K-group g', under scale codes 127 + g'.  Then
// C[row][c] = 2^(4 sigma + g') * (1 or 3): g', p' name k, sigma is the K-group whose scale the element took.
static void probe_kmap() {
    for (int side = 0; side < 2; side++) {
        for (int fmt = 0; fmt < 5; fmt++) {
            int kmap[4][32], smap[4][32];
            bool clean = true;
            for (int round = 0; round < 8; round++) {                                    // 16 (g, p) per launch, one per row
                Operands op; clear(op);
                uint32_t (*t)[8] = side == 0 ? op.a : op.b;
                uint32_t (*f)[8] = side == 0 ? op.b : op.a;
                uint32_t* ts = side == 0 ? op.sa : op.sb;
                uint32_t* fs = side == 0 ? op.sb : op.sa;
                for (int l = 0; l < 64; l++) {
                    const int r = l & 15, g = l >> 4, item = 16 * round + r;             // item = 32 g + p
                    if ((item >> 5) == g) put(t[l], kBits[fmt], item & 31, kOne[fmt]);
                    ts[l] = 127 + 4 * g;
                    put(f[l], 4, r, 0x2); put(f[l], 4, r + 16, 0x5);                     // E2M1 1.0 and 3.0
                    fs[l] = 127 + g;
                }
                float c[16][16];
                run(side == 0 ? fmt : E2M1, side == 0 ? E2M1 : fmt, op, c);
                for (int r = 0; r < 16; r++) {
                    const int item = 16 * round + r;
                    int hits = 0;
                    for (int q = 0; q < 16; q++) {
                        const float v = side == 0 ? c[r][q] : c[q][r];
                        if (v == 0.f) continue;
                        int e; const float m = std::frexp(v, &e);                        // v = m 2^e, m = 0.5 (1.0) or 0.75 (3.0)
                        const int three = m == 0.75f, ex = e - 1 - three;
                        if (m != 0.5f && m != 0.75f) clean = false;
                        kmap[item >> 5][item & 31] = 32 * (ex & 3) + q + 16 * three;
                        smap[item >> 5][item & 31] = ex >> 2;
                        hits++;
                    }
                    if (hits != 1) clean = false;
                }
            }
            printf("kmap    %s as %c%s\n", kNames[fmt], side == 0 ? 'A' : 'B', clean ? "" : "   (NOT one clean hit per element)");
            for (int g = 0; g < 4; g++) {
                printf("kmap      K-group %d: k =", g);
                for (int p = 0; p < 32; p++) printf(" %d", kmap[g][p]);
                printf("   scale of K-group");
                for (int p = 0; p < 32; p++) printf(" %d", smap[g][p]);
                printf("\n");
            }
        }
    }
}

static void probe_kgroup() {
    Operands op; clear(op);
    for (int l = 0; l < 64; l++) {
        const int r = l & 15, g = l >> 4;
        if (g == (r & 3)) fill(op.a[l], E4M3, kOne[E4M3]);                               // row r lives in group r & 3 only
        if (g == (r >> 2)) fill(op.b[l], E4M3, kOne[E4M3]);                              // column c in group c >> 2 only
    }
    float c[16][16];
    run(E4M3, E4M3, op, c);
    bool ok = true;
    for (int r = 0; r < 16; r++)
        for (int q = 0; q < 16; q++) ok = ok && c[r][q] == ((r & 3) == (q >> 2) ? 32.f : 0.f);
    printf("kgroup  lane l holds row / column l & 15, K-group l >> 4; C is column = lane & 15, row = 4 (lane >> 4) + reg: %s\n", ok ? "yes" : "NO");
}

template <int OP>
static void probe_opsel_one() {
    for (int side = 0; side < 2; side++) {
        Operands op; clear(op);
        for (int l = 0; l < 64; l++) {
            fill(op.a[l], E4M3, kOne[E4M3]);
            if ((l >> 4) == 0) fill(op.b[l], E4M3, kOne[E4M3]);
            (side == 0 ? op.sa : op.sb)[l] = 128u | (129u << 8) | (130u << 16) | (131u << 24);     // 2, 4, 8, 16
        }
        float c[16][16];
        if (side == 0) run_t<E4M3, E4M3, OP, 0>(op, c); else run_t<E4M3, E4M3, 0, OP>(op, c);
        printf("opsel   %c opsel %d: 32 x scale = %g -> byte %d of the scale register\n", side == 0 ? 'A' : 'B', OP, c[0][0], (int)std::log2(c[0][0] / 32.f) - 1);
    }
}

static void probe_scale() {
    Operands op; clear(op);
    for (int l = 0; l < 64; l++) {
        const int r = l & 15, g = l >> 4;
        fill(op.a[l], E2M1, kOne[E2M1]);
        if (g == 2) fill(op.b[l], E2M1, kOne[E2M1]);                                     // only K-group 2 counts
        op.sa[l] = 100 + 16 * g + r;                                                     // a code per lane
        op.sb[l] = 120 + 4 * g + (r & 3);
    }
    float c[16][16];
    run(E2M1, E2M1, op, c);
    bool ok = true;
    for (int r = 0; r < 16; r++)
        for (int q = 0; q < 16; q++) ok = ok && c[r][q] == std::ldexp(32.f, (100 + 32 + r - 127) + (120 + 8 + (q & 3) - 127));
    printf("scale   the code of lane (row, K-group) scales that lane's 32 elements only, A and B: %s\n", ok ? "yes" : "NO");
    clear(op);
    for (int l = 0; l < 64; l++) {
        if ((l >> 4) == 0) { fill(op.a[l], E4M3, kOne[E4M3]); fill(op.b[l], E4M3, kOne[E4M3]); }
        op.sa[l] = (l & 15) == 0 ? 0 : 254; op.sb[l] = (l & 15) == 0 ? 254 : 0;
    }
    run(E4M3, E4M3, op, c);
    printf("scale   codes 0 x 254: 32 x 2^-127 x 2^127 = %g (32 is exact); 0 x 0: %g; 254 x 254: %g\n", c[0][0], c[0][1], c[1][0]);
}

static void show_nan(const char* what, const float (&c)[16][16]) {
    int rows = 0, cols = 0, nans = 0;
    for (int r = 0; r < 16; r++) { bool any = false; for (int q = 0; q < 16; q++) { any = any || std::isnan(c[r][q]); nans += std::isnan(c[r][q]); } rows += any; }
    for (int q = 0; q < 16; q++) { bool any = false; for (int r = 0; r < 16; r++) any = any || std::isnan(c[r][q]); cols += any; }
    printf("nan     %-46s [3][5] = %g (0x%08x)  [3][0] = %g  [0][5] = %g  [0][0] = %g   NaN outputs: %d in %d rows, %d columns\n", what, c[3][5], bits_of(c[3][5]),
           c[3][0], c[0][5], c[0][0], nans, rows, cols);
}

static void probe_nan() {
    // everything 1.0 in K-group 0 (32 per output); the poison sits in row 3 of A (lane 3) unless stated
    auto base = [](Operands& op, int fa, int fb) {
        clear(op);
        for (int l = 0; l < 16; l++) { fill(op.a[l], fa, kOne[fa]); fill(op.b[l], fb, kOne[fb]); }
    };
    Operands op; float c[16][16];
    base(op, E2M1, E2M1); op.sa[3] = 0xff; run(E2M1, E2M1, op, c); show_nan("scale 0xFF on row 3 of A (FP4)", c);
    base(op, E2M1, E2M1); op.sb[5] = 0xff; run(E2M1, E2M1, op, c); show_nan("scale 0xFF on column 5 of B (FP4)", c);
    base(op, E2M1, E2M1); op.sa[3] = 0xff; memset(op.a[3], 0, sizeof(op.a[3])); run(E2M1, E2M1, op, c); show_nan("scale 0xFF on row 3 of A, its elements zero", c);
    base(op, E2M1, E2M1); op.sa[16 + 3] = 0xff; run(E2M1, E2M1, op, c); show_nan("scale 0xFF on row 3, K-group 1 (all zero elements)", c);
    base(op, E4M3, E4M3); op.a[3][0] = (op.a[3][0] & ~0xffu) | 0x7f; run(E4M3, E4M3, op, c); show_nan("E4M3 NaN code 0x7f in row 3 of A", c);
    base(op, E4M3, E4M3); op.a[3][0] = (op.a[3][0] & ~0xffu) | 0xff; run(E4M3, E4M3, op, c); show_nan("E4M3 NaN code 0xff in row 3 of A", c);
    base(op, E5M2, E4M3); op.a[3][0] = (op.a[3][0] & ~0xffu) | 0x7e; run(E5M2, E4M3, op, c); show_nan("E5M2 NaN code 0x7e in row 3 of A", c);
    base(op, E4M3, E5M2); op.b[5][0] = (op.b[5][0] & ~0xffu) | 0x7d; run(E4M3, E5M2, op, c); show_nan("E5M2 NaN code 0x7d in column 5 of B", c);
    base(op, E5M2, E4M3); op.a[3][0] = (op.a[3][0] & ~0xffu) | 0x7c; run(E5M2, E4M3, op, c); show_nan("E5M2 +Inf code 0x7c in row 3 of A", c);
    base(op, E5M2, E4M3); op.a[3][0] = (op.a[3][0] & ~0xffu) | 0xfc; run(E5M2, E4M3, op, c); show_nan("E5M2 -Inf code 0xfc in row 3 of A", c);
    base(op, E5M2, E4M3); op.a[3][0] = (op.a[3][0] & ~0xffffu) | 0xfc7c; run(E5M2, E4M3, op, c); show_nan("E5M2 +Inf and -Inf in row 3 of A", c);
    base(op, E5M2, E4M3); op.a[3][0] = (op.a[3][0] & ~0xffu) | 0x7c; op.b[5][0] &= ~0xffu; run(E5M2, E4M3, op, c); show_nan("E5M2 +Inf in row 3 times 0 in column 5", c);
}

static void probe_width() {
    // row 0 of A (E5M2): 2^e and -2^e in block 0 (an element 2^15 under scale code 127 + e - 15), 1.0 in block 1 under scale code
    // 127, against ones: the exact sum is 1.  By kmap an FP8 lane group 0 holds k = 0 .. 15 and group 2 holds k = 32 .. 47.
    for (int e = 20; e <= 40; e += 4) {
        Operands op; clear(op);
        fill(op.b[0], E4M3, kOne[E4M3]);
        fill(op.b[32], E4M3, kOne[E4M3]);
        put(op.a[0], 8, 0, 0x78);                                                        // E5M2 2^15
        put(op.a[0], 8, 1, 0xf8);                                                        // -2^15
        op.sa[0] = 127 + (e - 15);
        put(op.a[32], 8, 0, 0x3c);                                                       // 1.0 at k = 32: block 1, scale of lane group 1
        float c[16][16];
        run(E5M2, E4M3, op, c);
        float d[16][16];
        op.a[0][0] = 0x78;                                                               // without the -2^e: 2^e + 1
        run(E5M2, E4M3, op, d);
        printf("width   one instruction: 2^%d - 2^%d + 1 = %g;   2^%d + 1 = 2^%d + %g\n", e, e, c[0][0], e, e, d[0][0] - std::ldexp(1.f, e));
    }
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    printf("# tools/mx_mfma_probe on %s (%s)\n", prop.name, prop.gcnArchName);
    CHECK(hipMalloc(&d_in, sizeof(Operands)));
    CHECK(hipMalloc(&d_out, 256 * sizeof(float)));
    probe_order();
    probe_kmap();
    probe_kgroup();
    probe_opsel_one<0>(); probe_opsel_one<1>(); probe_opsel_one<2>(); probe_opsel_one<3>();
    probe_scale();
    probe_nan();
    probe_width();
    CHECK(hipDeviceSynchronize());
    CHECK(hipFree(d_in)); CHECK(hipFree(d_out));
    return 0;
}
