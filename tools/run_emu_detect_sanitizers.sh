#!/bin/bash
# The source-finding kernels (spx_detect_kernels.h) on the CPU harness (tests/cpu_emu/emu_detect.cpp) under
# the address/UB sanitizers (LDS is a heap block of exactly the launch's size: any out-of-range LDS or global
# access is reported) and under ThreadSanitizer (a missing barrier or a non-atomic access inside the LDS
# union-find is a data race).  Runs tests/test_detect_cpu.py against each build; exit code 1 on any report.
#   tools/run_emu_detect_sanitizers.sh [asan|tsan]      (default: both)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
FLAGS=$(make -s -C subpixal_amd/csrc --eval 'spx-emu-flags: ; @echo $(HOSTCXX) $(EMUFLAGS)' spx-emu-flags)
OUT=tests/cpu_emu/build
mkdir -p $OUT
WHAT=${1:-both}
if [ "$WHAT" != tsan ]; then
    $FLAGS -fsanitize=address,undefined -fno-omit-frame-pointer -shared-libsan -shared \
        -o $OUT/libspx_emu_detect_asan.so tests/cpu_emu/emu_detect.cpp
    RT=$(ls /opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so | head -1)
    ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 LD_PRELOAD="$RT" \
    SPX_EMU_DETECT_LIB="$ROOT/$OUT/libspx_emu_detect_asan.so" python -m pytest tests/test_detect_cpu.py -x -q
fi
if [ "$WHAT" != asan ]; then
    $FLAGS -fsanitize=thread -shared-libsan -shared -o $OUT/libspx_emu_detect_tsan.so tests/cpu_emu/emu_detect.cpp
    RT=$(ls /opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.tsan-x86_64.so | head -1)
    LOG=$(mktemp)
    # the 648-source domino scene is left out here: one workgroup per source, 10-20x slower under this sanitizer
    TSAN_OPTIONS="halt_on_error=0 report_signal_unsafe=0 history_size=4" LD_PRELOAD="$RT" \
    SPX_EMU_DETECT_LIB="$ROOT/$OUT/libspx_emu_detect_tsan.so" python -m pytest tests/test_detect_cpu.py -x -q \
        -k "not domino" > "$LOG" 2>&1 || { tail -30 "$LOG"; exit 1; }
    grep -v "^==\|^$" "$LOG" | tail -5
    N=$(grep -c "WARNING: ThreadSanitizer" "$LOG" || true)
    echo "ThreadSanitizer reports: $N"
    test "$N" = "0"
fi
