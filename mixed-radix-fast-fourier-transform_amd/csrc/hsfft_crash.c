/*
 * hsfft_crash.c -- HSFFT_CRASH_TRACE diagnostics of libhsfft.so (host C, self-contained).
 */
#define _GNU_SOURCE
#include <execinfo.h>
#include <fcntl.h>
#include <signal.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>
#include <unistd.h>

#include "hsfft_host.h"

/* HSFFT_CRASH_TRACE=1 (diagnostics): on SIGSEGV / SIGBUS / SIGILL / SIGFPE / SIGABRT the
 * library writes the signal, the faulting address and instruction pointer, the native
 * backtrace (library + offset per frame) and /proc/self/maps to stderr, then re-raises the
 * signal with its default action.  Installed when the library is loaded and again when a
 * device is selected (a tool that installs its own handler while the runtime initialises would
 * otherwise replace it). */
static void crash_puts(const char *s)
{
    size_t n = strlen(s);
    while (n > 0) {
        const ssize_t w = write(2, s, n);
        if (w <= 0) return;
        s += w;
        n -= (size_t)w;
    }
}

static void crash_hex(const char *label, unsigned long long v)
{
    char b[40];
    int i = 39;
    b[i] = 0;
    do {
        b[--i] = "0123456789abcdef"[v & 15];
        v >>= 4;
    } while (v && i > 2);
    b[--i] = 'x';
    b[--i] = '0';
    crash_puts(label);
    crash_puts(b + i);
}

static void crash_handler(int sig, siginfo_t *si, void *ucv)
{
    crash_hex("\n*** hsfft crash trace: signal ", (unsigned long long)sig);
    crash_hex(" fault address ", (unsigned long long)(uintptr_t)si->si_addr);
#if defined(__x86_64__)
    const ucontext_t *uc = (const ucontext_t *)ucv;
    crash_hex(" rip ", (unsigned long long)uc->uc_mcontext.gregs[REG_RIP]);
#else
    (void)ucv;
#endif
    crash_puts("\n*** backtrace:\n");
    void *fr[64];
    const int n = backtrace(fr, 64);
    backtrace_symbols_fd(fr, n, 2);
    crash_puts("*** /proc/self/maps:\n");
    const int fd = open("/proc/self/maps", O_RDONLY);
    if (fd >= 0) {
        char buf[4096];
        ssize_t r;
        while ((r = read(fd, buf, sizeof buf)) > 0)
            if (write(2, buf, (size_t)r) != r) break;
        close(fd);
    }
    crash_puts("*** end of hsfft crash trace\n");
    signal(sig, SIG_DFL);
    raise(sig);
}

void hs_crash_trace_install(void)
{
    const char *e = getenv("HSFFT_CRASH_TRACE");
    if (!e || !atoi(e)) return;
    void *warm[2];
    (void)backtrace(warm, 2); /* loads the unwinder now, not inside the handler */
    struct sigaction sa;
    memset(&sa, 0, sizeof sa);
    sa.sa_sigaction = crash_handler;
    sa.sa_flags = SA_SIGINFO;
    sigemptyset(&sa.sa_mask);
    const int sigs[] = {SIGSEGV, SIGBUS, SIGILL, SIGFPE, SIGABRT};
    for (unsigned i = 0; i < sizeof sigs / sizeof sigs[0]; i++) sigaction(sigs[i], &sa, NULL);
}

__attribute__((constructor)) static void crash_trace_ctor(void) { hs_crash_trace_install(); }
