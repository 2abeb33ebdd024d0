// TEST-ONLY shim over the host emulation (tests/emu/emu.cpp, compiled in here with the
// NTC_STAT counters on): the host-built path stream with its substitution words
// (encode_core.h subst_clean, derived.cpp build_tab_host) and the counters of the
// substitution shortcut in MsLaneT<false>::step.  Used by tests/test_subst.py only.
#include "../emu/emu.cpp"

#if !defined(__HIP_DEVICE_COMPILE__)
uint64_t ntc::ntc_stats[16];

// NTC_STAT counters since the last call (13: shortcut taken, 14: unconfirmed guess fell back)
extern "C" void subst_stats(uint64_t *out) {
    for (int i = 0; i < 16; i++) out[i] = ntc_stats[i];
    memset(ntc_stats, 0, sizeof ntc_stats);
}
#endif

// The path stream as the emulator's index holds it (NTC_EMU_JOINT, NTC_SUBST apply): out =
// groups x {chars lo, chars hi, end bits, substitution word}.  info = {groups, text length,
// U, tab_pos, t_jump, subst_word_hash}.  Returns 0, 1 (bad index), 2 (no path cover), 3 (cap).
extern "C" int subst_host_words(const ntc_index_view *v, uint32_t tab_u, uint32_t *out, uint64_t cap, uint64_t *info) {
    HostIndex hx;
    Derived dv;
    std::vector<WalkEntry> walk;
    DevIndex d{};
    std::vector<uint2> tab;
    std::vector<uint32_t> bits, fbits;
    std::vector<uint16_t> pairb;
    if (!load(v, hx, dv, walk, d, tab, bits, fbits, pairb, tab_u)) return 1;
    if (!dv.has_paths) return 2;
    const uint64_t groups = pstream_groups(dv.tlen, hx.k);
    info[0] = groups;
    info[1] = dv.tlen;
    info[2] = d.tab_u;
    info[3] = d.tab_pos;
    info[4] = dv.t_jump;
    info[5] = subst_word_hash(dv.pstream.data(), groups);
    if (groups * 4 > cap) return 3;
    for (uint64_t g = 0; g < groups; g++) {
        out[4 * g] = dv.pstream[g].x;
        out[4 * g + 1] = dv.pstream[g].y;
        out[4 * g + 2] = dv.pstream[g].z;
        out[4 * g + 3] = dv.pstream[g].w;
    }
    return 0;
}
