// TEST INFRASTRUCTURE ONLY -- libslimm_emu.so for a command whose host threads drive several contexts at once
// (slimm --file-per-device under ThreadSanitizer, scripts/sanitize_host.sh).  The emulator's scheduler and its state are one
// per process: two host threads that launch kernels at the same moment end it with "nested kernel launch".  This library is
// linked against libslimm_emu.so and is what SLIMM_HIP_LIB names instead of it: the command finds every slimm_* symbol
// through it, and hipemu::launch below comes before the emulator's own in the look-up order of the two, so the emulator's
// kernels launch through here -- one at a time, whichever thread asks.
// Built by scripts/sanitize_host.sh: g++ -shared -fPIC -I hip_emu emu_one_launch.cpp -L. -Wl,--no-as-needed -lslimm_emu -ldl
// (--no-as-needed: nothing here names a symbol of the emulator, and the command must find them through this library).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>

namespace hipemu {
void launch(dim3 grid, dim3 block, size_t shmem, const std::function<void()>& body) {
    using Launch = void (*)(dim3, dim3, size_t, const std::function<void()>&);
    static const Launch next = reinterpret_cast<Launch>(dlsym(RTLD_NEXT, "_ZN6hipemu6launchE4dim3S0_mRKSt8functionIFvvEE"));
    if (!next) {
        std::fprintf(stderr, "emu_one_launch: the emulator's hipemu::launch was not found behind this library\n");
        std::abort();
    }
    // (recursive: a launch from inside a kernel still reaches the emulator's own message)
    static std::recursive_mutex one_at_a_time;
    std::lock_guard<std::recursive_mutex> guard(one_at_a_time);
    next(grid, block, shmem, body);
}
}  // namespace hipemu
