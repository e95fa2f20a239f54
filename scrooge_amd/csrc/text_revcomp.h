// text_revcomp.h — texts taken as the REVERSE COMPLEMENT of their stretch (scrg_ctx_set_text_strands, bit 63 of
// scrg_pair_desc.text_off: SCRG_TEXT_REVCOMP), from the one packed (forward) copy: the address arithmetic of that load, compiled
// for the device (the one-pair-per-lane kernels) and for the host (scrg_text_window_planes, which the CPU tests hold to a plain
// statement of the semantics and to the bounds below).
//
// text_off (bit 63 cleared) and text_len name a forward stretch; character k of the text is the complement of base
// text_off + text_len - 1 - k.  The 64 characters from character c on are therefore the 64 forward bases that END at
// text_len - c, read backwards and inverted in both planes (A0 C1 G2 T3): a window is loaded from `at` = that end - 64, not
// below 0 — a flagged pair never reads a word below the first word of its stretch — moved up by `sh` when fewer than 64 bases
// are left, bit-reversed and inverted.  `at` <= text_len, so on the high side the load stays where the loads of forward pairs
// (from ref_idx <= text_len) already go.
#pragma once

#include <stdint.h>

#include "genasm_kernels.h"

namespace scrg {

// A pair's text as the kernels use it: the flag taken out of the offset (only when the launch honours it), the length
// saturated to 32 bits.  The END of a flagged stretch is formed in 64 bits first: of a longer stretch the LAST 2^32 - 1 bases
// are the reachable ones, as the first ones are of a forward text.
struct TextStretch {
    uint64_t off;
    uint32_t len;
    bool rev;
};
SCRG_HD inline TextStretch text_stretch(uint64_t text_off, uint64_t text_len, bool enabled, uint32_t stride)
{
    TextStretch t;
    t.rev = enabled && (text_off & SCRG_TEXT_REVCOMP) != 0;
    t.off = enabled ? text_off & ~SCRG_TEXT_REVCOMP : text_off;
    t.len = text_len > 0xffffffffull ? 0xffffffffu : (uint32_t)text_len;
    if (t.rev && text_len > 0xffffffffull) {       // base (text_len - len) of the stretch becomes its first (scrooge_amd.h: scrg_pair_desc)
        const uint64_t inner = (t.off & 31u) + (text_len - t.len);
        t.off = (((t.off >> 5) + (inner >> 5) * stride) << 5) | (inner & 31u);
    }
    return t;
}

// Word w (characters 64 w .. 64 w + 63) of the window at ref_idx of a reversed text: made of the 64 forward bases from base
// `at` of the stretch, shifted up by `sh` (fewer than 64 left: the load starts at base 0).  A word past the text: at = 0.
struct TextRevAt {
    uint32_t at, sh;
};
SCRG_HD inline TextRevAt text_rev_at(uint32_t text_len, uint32_t ref_idx, uint32_t w)
{
    const uint32_t left = text_len > ref_idx ? text_len - ref_idx : 0u;
    const uint32_t end = left > 64u * w ? left - 64u * w : 0u;          // the word's forward window ends here (exclusive)
    TextRevAt r;
    r.at = end > 64u ? end - 64u : 0u;
    r.sh = (end >= 64u ? 0u : 64u - end) & 63u;
    return r;
}

// The first of the three words (`stride` words apart) that the load of 64 bases from base k of a sequence at `off` touches,
// and the bit of each plane at which base k sits in it: base k lives in word off/32 + ((off%32 + k)/32)*stride.  The loads that
// take a base offset (genasm_device.h: load_window_strided, load_window_words — every reversed load of the wide, parts and mw
// kernels among them) form their word index here; the default kernel's load_window_words_at and lane_multiword.h's load_planes
// start from a pointer to the sequence's first word, made once per pair, and add (in-word offset + k) / 32 * stride themselves.
SCRG_HD inline uint64_t window_first_word(uint64_t off, uint32_t k, uint32_t stride, uint32_t& bit)
{
    const uint32_t inner = ((uint32_t)off & 31u) + k;
    bit = inner & 31u;
    return (off >> 5) + (uint64_t)(inner >> 5) * stride;
}

}  // namespace scrg
