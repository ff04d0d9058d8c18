/* Lazy steepest-descent SE2 cell kernels: the one diagnostic of libipc_amd.so's C ABI that goes with them.
 *
 * Not a header to include by itself: include/ipc_amd.h includes it, behind ipc_engine_t.  ipc_amd.capi lists the name in
 * SYMBOLS_LAZY_SD. */
#ifndef IPC_AMD_LAZY_SD_H
#define IPC_AMD_LAZY_SD_H
#ifndef IPC_AMD_H
#error "include ipc_amd.h, which includes this header"
#endif

/* Launches, since ipc_create, of a lazy steepest-descent SE2 cell kernel in place of the wave / pair kernel a bin's policy
 * token names (same cells, same results bit for bit).  IPC_SE2_LAZY_SD=0 switches the substitution off: then 0. */
int ipc_se2_lazy_sd_launches(ipc_engine_t* h, long long* launches);

#endif
