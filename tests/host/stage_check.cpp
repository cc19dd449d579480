// stage_check.cpp -- the staging layout of the host text pipes (StageCursor of sigtk_amd/csrc/text_pipe.h) on its own
// (tests/test_stage_cpu.py builds it under -fsanitize=address,undefined): for the sections of the sref and the ss
// staging, over a grid of byte and element counts, the cursor's offsets equal the formulas the pipes' begin calls used to
// spell out, and every section starts 16-byte aligned.  Nothing here touches a device.
#include <stdio.h>

#include "text_pipe.h"

using sgk::round_up;

static int wrong = 0;
static void same(const char *what, size_t got, size_t want) {
    if (got == want && got % 16 == 0) return;
    if (++wrong <= 20) printf("%s: %zu, expected %zu\n", what, got, want);
}

int main() {
    const uint64_t bytes[] = {0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 1000003, (1ull << 32) - 1, (1ull << 40) + 3};
    const uint32_t counts[] = {0, 1, 15, 16, 17, 255, 256, 257, 0xfffffffeu, 0xffffffffu};
    long cases = 0;
    for (uint64_t n_text : bytes) {          // bases | ss strings
        for (uint64_t n_idb : bytes) {       // name bytes | id bytes
            for (uint32_t n_spans : counts) {
                for (uint32_t n_ids : counts) {  // names | ids
                    {  // sref: bases (+ 16) | spans | name bytes (+ 16) | name offsets
                        const size_t off_spans = round_up(n_text + 16, 16);
                        const size_t off_nbytes = round_up(off_spans + (size_t)n_spans * sizeof(sgk_sref_span_t), 16);
                        const size_t off_noffs = round_up(off_nbytes + n_idb + 16, 16);
                        const size_t in_bytes = round_up(off_noffs + ((size_t)n_ids + 1) * 4, 16);
                        sgk::StageCursor c;
                        same("sref bases", c.take(n_text, 16), 0);
                        same("sref spans", c.take((size_t)n_spans * sizeof(sgk_sref_span_t)), off_spans);
                        same("sref name bytes", c.take(n_idb, 16), off_nbytes);
                        same("sref name offsets", c.take(((size_t)n_ids + 1) * 4), off_noffs);
                        same("sref blob", c.pos, in_bytes);
                    }
                    for (uint32_t n_records : counts) {  // ss: strings (+ 16) | records | spans | id bytes (+ 16) | id offsets
                        const size_t off_rec = round_up(n_text + 16, 16);
                        const size_t off_spans = round_up(off_rec + (size_t)n_records * sizeof(sgk_ss_record_t), 16);
                        const size_t off_ids = round_up(off_spans + (size_t)n_spans * sizeof(sgk_ss_span_t), 16);
                        const size_t off_idoffs = round_up(off_ids + n_idb + 16, 16);
                        const size_t in_bytes = round_up(off_idoffs + ((size_t)n_ids + 1) * 4, 16);
                        sgk::StageCursor c;
                        same("ss strings", c.take(n_text, 16), 0);
                        same("ss records", c.take((size_t)n_records * sizeof(sgk_ss_record_t)), off_rec);
                        same("ss spans", c.take((size_t)n_spans * sizeof(sgk_ss_span_t)), off_spans);
                        same("ss id bytes", c.take(n_idb, 16), off_ids);
                        same("ss id offsets", c.take(((size_t)n_ids + 1) * 4), off_idoffs);
                        same("ss blob", c.pos, in_bytes);
                        ++cases;
                    }
                }
            }
        }
    }
    printf("%ld layouts: %d wrong\n", cases, wrong);
    return wrong != 0;
}
