/* mrp_host_pool.h -- the persistent host thread pool (mrp_host_pool.cpp) as the C++ side of the library sees it.  No HIP. */
#ifndef MRP_HOST_POOL_H_
#define MRP_HOST_POOL_H_

#include "rphmm_host.h" /* mrp_pool_run, mrp_pool_adopt, mrp_host_threads, mrp_set_error, the status codes */

int mrp_host_threads_setting(void); /* what mrp_set_host_threads() was given, 0 if it was never called */
struct mrp_host_pool;
mrp_host_pool *mrp_host_pool_create(int threads);
void mrp_host_pool_destroy(mrp_host_pool *p);
template <class F>
static inline void mrp_parallel_for(int64_t n, int64_t grain, F f) {
    mrp_pool_run(n, grain, [](int64_t i, void *a) { (*static_cast<F *>(a))(i); }, &f);
}

#endif
