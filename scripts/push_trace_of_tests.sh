#!/bin/sh
# What the window pipeline planned, reserved, launched and finished (SLIMM_TRACE=push) while the tests that cover its input
# forms ran under the host emulator, with everything that varies from run to run taken out (the time stamps, the two
# timing payloads).  Under the emulator the rest is deterministic, so for a change that should not alter the pipeline's
# decisions:
#     scripts/push_trace_of_tests.sh > after.txt
#     scripts/push_trace_of_tests.sh /path/to/a/checkout/of/the/parent > before.txt
#     diff before.txt after.txt          # empty
# (the forms: BGZF BAM with and without a size hint, plain SAM, BGZF SAM without its last newline, bzip2 SAM in rounds small
# enough to cut blocks)
set -eu
root=${1:-$(cd "$(dirname "$0")/.." && pwd)}
cd "$root"
make -s -C tests/native -j8 >&2
SLIMM_EMU=1 SLIMM_TRACE=push python -m pytest -q -s -p no:cacheprovider -m gpu \
    tests/test_gpu_bgzf_inflate.py tests/test_gpu_sam_decode.py tests/test_gpu_compressed_sam.py tests/test_gpu_bzip2_sam.py \
    -k "test_window_buffers_are_sized_by_the_file or test_grouped_text_decoded_on_the_device or \
        test_last_line_without_newline_inflated_on_the_device or \
        (test_bzip2_sam_bytes_give_the_partials_of_the_text and level1 and (random or 60k))" 3>&2 2>&1 >&3 3>&- |
    grep '^\[push' |
    sed -E -e 's/^\[push +[0-9.]+\] /[push] /' -e 's/(page-locked [0-9]+ MB) in [0-9.]+ ms/\1/' -e 's/(false magics); find .* ms$/\1/'
