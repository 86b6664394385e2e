// devbuf_rule.h -- how large the engine's growable device buffers are made, stated once (devbuf.h, engine.hip).  Plain
// C++ with no device call, so that it also builds into a stand-alone host program.
//
// A buffer regrows only when a call needs more elements than it holds; it is then allocated anew at the size below, the
// old contents dropped.  Every count is in ELEMENTS of the buffer (floats of feat and nat, ints of first and nat_row):
// a stream row is layersizes[0] / fea_context floats wide and fea_context is an argument of every call, so a count of
// rows says nothing about what feat and nat hold.
#pragma once
#include <stddef.h>

namespace devbuf_rule {

// rows of a raw set's target stream (D floats each) for a stream of `rows` rows read through windows of ctx rows
inline size_t raw_rows(size_t rows, size_t ctx) { return rows + ctx + 8; }
// floats of its feature stream, rows of fdim floats
inline size_t raw_feat_floats(size_t rows, size_t ctx, size_t fdim) { return raw_rows(rows, ctx) * fdim; }
// floats of a NAT engine's noise table of n_nat rows
inline size_t nat_floats(size_t n_nat, size_t fdim) { return (n_nat + 8) * fdim; }
// entries of a per-sample table (first, nat_row) and rows of the expanded chunk buffers of n samples: the padded tiles
// of the last bunch (Bp rows) may read past the last sample
inline size_t sample_slots(size_t n, size_t Bp) { return n + Bp + 32; }
// rows of chunk_out for the outputs of n_frames frames
inline size_t out_rows(size_t n_frames) { return n_frames + 32; }
// floats of the learned scale's state (scale_rule.h): two copies of (alpha, v) per padded output unit
inline size_t scale_state_floats(size_t Dp) { return 2 * 2 * Dp; }
// bytes of a workspace buffer that has to hold `bytes`: an eighth of headroom, so that batches of slightly different
// sizes settle after the first few
inline size_t ws_bytes(size_t bytes) { return bytes + bytes / 8 + 256; }

// does a call that needs `need` elements regrow a buffer that holds `cap` (DevBuf::grow asks exactly this)
inline bool regrows(size_t need, size_t cap) { return need > cap; }

// the capacity of one buffer under the rule, without the buffer: what a host program can follow through a call sequence
struct Cap {
    size_t cap = 0;
    bool grow(size_t need, size_t alloc) {
        if (!regrows(need, cap)) return false;
        cap = alloc;
        return true;
    }
};

}  // namespace devbuf_rule
