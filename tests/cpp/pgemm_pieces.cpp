// pgemm_pieces — the prefill GEMM's LDS-DMA piece addresses (csrc/prefill.h pg_piece, PgGeo::piece / dst), checked on
// the host before any GPU run. For every tiling pg_pick returns (3 weight types x 3 roles x 4 chunk sizes) and K in
// {64, 128, 192, 320, 704}, every piece of every stage, wave and lane is enumerated:
//   - its 16-byte (scale piece: 1-byte) source range lies inside its own row's K bytes;
//   - every piece of the stage image is issued by exactly one wave, and no LDS byte is written twice;
//   - every byte of every valid k-block sits at the LDS offset the kernel's fragment reads take it from.
// No device code runs: main() only calls the __host__ __device__ address functions.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "prefill.h"

using namespace sli;

static int g_fail = 0;
static long g_pieces = 0;

#define EXPECT(cond, ...)                    \
    do {                                     \
        if (!(cond)) {                       \
            if (g_fail++ < 20) {             \
                fprintf(stderr, __VA_ARGS__); \
                fprintf(stderr, "\n");       \
            }                                \
        }                                    \
    } while (0)

struct Byte {  // what an LDS byte holds: byte `at` of row `row`'s K bytes of operand `kind` (-1: not written)
    int kind = -1, row = 0;
    long at = 0;
    bool is(int k, int r, long a) const { return kind == k && row == r && at == a; }
};

template <class Cfg, typename WT>
static void check(const char* wt, int role, int M, int K) {
    using Geo = PgGeo<Cfg, WT>;
    using F = typename Geo::F;
    constexpr int KBS = Geo::KBS, NA = Geo::NA;
    const int ns = (K + Geo::KS - 1) / Geo::KS, kt = K % Geo::KS;
    const int vkb = kt ? kt / 32 : KBS;  // k-blocks of the last stage
    const long row_bytes[4] = {(long)wt_row_bytes<WT>(K), 2L * K, 2L * K, K / kMxBlock};
    const int rows[4] = {NA * 16, Geo::BM, Geo::BM, NA * 16};
    char tag[96];
    snprintf(tag, sizeof tag, "%s role %d M %d BM %d WR %d S %d AT %d SA %d K %d", wt, role, M, Geo::BM, Geo::WR, Geo::S,
             Geo::AT, Geo::SA, K);
    for (int s = 0; s < ns; ++s) {
        const bool tail = kt && s == ns - 1;
        std::vector<Byte> lds(Geo::STAGE);
        std::vector<int> issued(Geo::NP, 0);
        for (int w = 0; w < Geo::WAVES; ++w)
            for (int j = 0; j < Geo::DPW; ++j) {
                const int d = Geo::piece(w, j);
                EXPECT(d >= 0 && d < Geo::NP, "%s: wave %d piece %d -> %d outside the stage", tag, w, j, d);
                if (d < 0 || d >= Geo::NP) continue;
                ++issued[d];
                ++g_pieces;
                for (int lane = 0; lane < 64; ++lane) {
                    const PgPiece p = pg_piece<Geo>(d, lane, vkb);
                    const int n = p.kind == 3 ? 1 : 16;  // bytes the lane moves
                    EXPECT(p.kind >= 0 && p.kind <= 3 && (F::SCALED || p.kind != 3), "%s: piece %d kind %d", tag, d, p.kind);
                    if (p.kind < 0 || p.kind > 3) continue;
                    EXPECT(p.row >= 0 && p.row < rows[p.kind], "%s: piece %d lane %d row %d", tag, d, lane, p.row);
                    const long at = p.at(s, tail);
                    EXPECT(at >= 0 && at + n <= row_bytes[p.kind], "%s: stage %d piece %d lane %d kind %d reads [%ld, %ld) of %ld",
                           tag, s, d, lane, p.kind, at, at + n, row_bytes[p.kind]);
                    const int dst = Geo::dst(d) + lane * (p.kind == 3 ? 4 : 16);
                    EXPECT(dst >= 0 && dst + n <= Geo::STAGE, "%s: piece %d lane %d lands at %d of %d", tag, d, lane, dst,
                           Geo::STAGE);
                    if (dst < 0 || dst + n > Geo::STAGE) continue;
                    for (int i = 0; i < n; ++i) {
                        EXPECT(lds[dst + i].kind == -1, "%s: stage %d LDS byte %d written twice", tag, s, dst + i);
                        lds[dst + i].kind = p.kind;
                        lds[dst + i].row = p.row;
                        lds[dst + i].at = at + i;
                    }
                }
            }
        for (int d = 0; d < Geo::NP; ++d) EXPECT(issued[d] == 1, "%s: piece %d issued %d times", tag, d, issued[d]);
        // the fragment reads of the stage's valid k-blocks (pgemm_kernel read_frags), lane = 16 kg + r
        const int kbs = s == ns - 1 ? vkb : KBS;
        for (int kb = 0; kb < kbs; ++kb)
            for (int r = 0; r < 16; ++r)
                for (int kg = 0; kg < 4; ++kg) {
                    const int k = 32 * kb + 8 * kg;  // the lane's 8 k of the stage
                    for (int ti = 0; ti < NA; ++ti) {
                        const int o = ti * Geo::A_IMG + r * Geo::A_ROW + F::a_off(kb, kg, F::swz(r));
                        const long at = (long)s * Geo::A_ROW + k * Geo::A_ROW / Geo::KS;
                        for (int i = 0; i < F::FRAG; ++i)
                            EXPECT(lds[o + i].is(0, ti * 16 + r, at + i), "%s: stage %d A tile %d row %d kb %d kg %d byte %d", tag,
                                   s, ti, r, kb, kg, i);
                    }
                    for (int u = 0; u < 2 * Geo::PT; ++u) {  // image 2 pt + (lo ? 1 : 0)
                        const int o = Geo::A_BYTES + u * Geo::B_IMG + r * Geo::B_ROW + ((4 * kb + kg) ^ pg_swz(r, Geo::B_ROW)) * 16;
                        const long at = (long)s * Geo::B_ROW + 2 * k;
                        for (int i = 0; i < 16; ++i)
                            EXPECT(lds[o + i].is(1 + (u & 1), (u >> 1) * 16 + r, at + i), "%s: stage %d B image %d row %d kb %d kg %d byte %d",
                                   tag, s, u, r, kb, kg, i);
                    }
                    if (F::SCALED)  // the lane's C rows 4 kg .. +4 of each tile: one 16-byte read, a scale per dword
                        for (int ti = 0; ti < NA; ++ti)
                            for (int e = 0; e < 4 && r == 0; ++e) {
                                const int o = Geo::A_BYTES + Geo::B_BYTES + ((kb * NA + ti) * 16 + 4 * kg + e) * 4;
                                EXPECT(lds[o].is(3, ti * 16 + 4 * kg + e, (long)s * KBS + kb), "%s: stage %d scale tile %d row %d kb %d",
                                       tag, s, ti, 4 * kg + e, kb);
                            }
                }
    }
}

template <typename WT>
static void check_type(const char* wt) {
    const int Ks[] = {64, 128, 192, 320, 704};
    for (int M : kPfSizes)
        for (int role = 0; role < 3; ++role)
            for (int K : Ks)
                pg_pick<WT>(M, role, [&](auto cfg) {
                    check<decltype(cfg), WT>(wt, role, M, K);
                    return 0;
                });
}

int main() {
    check_type<__half>("f16");
    check_type<int8_t>("i8");
    check_type<mxfp4>("mxfp4");
    if (g_fail) {
        fprintf(stderr, "pgemm_pieces: %d failures\n", g_fail);
        return 1;
    }
    printf("pgemm_pieces: %ld pieces ok\n", g_pieces);
    return 0;
}
