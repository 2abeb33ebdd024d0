// TEST-ONLY shim over the host emulation (tests/emu/emu.cpp, compiled in here): the arrays
// the emulator's load() derives from an index view on the host -- walk table, rank chunks,
// suffix table, presence bitmaps, pair words, window words -- and the host path cover's
// pos_of_node and text, so that tests/test_derived.py can hold them against a definition
// written without the shared per-entry functions, and tests/test_gpu_derived.py against the
// arrays the upload builds on the device.  Used by those two tests only.
#include "../emu/emu.cpp"

namespace {
struct Held {
    HostIndex hx;
    Derived dv;
    std::vector<WalkEntry> walk;
    DevIndex d{};
    std::vector<uint2> tab;
    std::vector<uint32_t> bits, fbits;
    std::vector<uint16_t> pairb;
} g_held;
}  // namespace

enum { kDvWalk, kDvRank2, kDvTab, kDvBits, kDvFbits, kDvPair, kDvWin, kDvPos, kDvPstream, kDvArrays };

// Builds and holds the arrays of one index (NTC_EMU_EXT2=1 for the rank chunks; the other
// NTC_EMU_* switches of load() apply).  info = {U, tab_pos, t_jump, has_paths, path text
// length, filter level, absent mask, n} then the byte size of each array by the enum above
// (0: not built).  Returns 0, or 1 for a bad index.
extern "C" int derived_host_build(const ntc_index_view *v, uint32_t tab_u, uint64_t *info) {
    Held &h = g_held;
    if (!load(v, h.hx, h.dv, h.walk, h.d, h.tab, h.bits, h.fbits, h.pairb, tab_u)) return 1;
    const uint32_t U = h.d.tab_u;
    info[0] = U;
    info[1] = h.d.tab_pos;
    info[2] = h.dv.t_jump;
    info[3] = h.dv.has_paths;
    info[4] = h.dv.tlen;
    info[5] = filter_level(U);
    info[6] = h.dv.absent;
    info[7] = h.hx.n;
    uint64_t *sz = info + 8;
    sz[kDvWalk] = h.walk.size() * sizeof(WalkEntry);
    sz[kDvRank2] = h.d.rank2 ? rank2_blocks(h.hx.n) * 4 * sizeof(Rank2Chunk) : 0;
    sz[kDvTab] = h.tab.size() * sizeof(uint2);
    sz[kDvBits] = h.bits.size() * 4;
    sz[kDvFbits] = h.fbits.size() * 4;
    sz[kDvPair] = h.d.pair_w ? h.pairb.size() * 2 : 0;
    sz[kDvWin] = h.d.win_w ? win_words_count(U) * 32 : 0;
    sz[kDvPos] = h.dv.pos_of_node.size() * 4;
    sz[kDvPstream] = h.dv.pstream.size() * sizeof(uint4);
    return 0;
}

// Copies array `which` of the last derived_host_build into out (exactly `bytes` bytes, the
// size that call reported).  Returns 0, 2 (unknown array or not built), 3 (size mismatch).
extern "C" int derived_host_get(int which, void *out, uint64_t bytes) {
    const Held &h = g_held;
    const void *p = nullptr;
    uint64_t have = 0;
    switch (which) {
    case kDvWalk: p = h.walk.data(), have = h.walk.size() * sizeof(WalkEntry); break;
    case kDvRank2: p = h.d.rank2, have = p ? rank2_blocks(h.hx.n) * 4 * sizeof(Rank2Chunk) : 0; break;
    case kDvTab: p = h.tab.data(), have = h.tab.size() * sizeof(uint2); break;
    case kDvBits: p = h.bits.data(), have = h.bits.size() * 4; break;
    case kDvFbits: p = h.fbits.data(), have = h.fbits.size() * 4; break;
    case kDvPair: p = h.d.pair_w, have = p ? h.pairb.size() * 2 : 0; break;
    case kDvWin: p = h.d.win_w, have = p ? win_words_count(h.d.tab_u) * 32 : 0; break;
    case kDvPos: p = h.dv.pos_of_node.data(), have = h.dv.pos_of_node.size() * 4; break;
    case kDvPstream: p = h.dv.pstream.data(), have = h.dv.pstream.size() * sizeof(uint4); break;
    default: return 2;
    }
    if (!p || !have) return 2;
    if (have != bytes) return 3;
    memcpy(out, p, bytes);
    return 0;
}
