// set_full_scan.h -- the four launches of set_full.hip, the unit that holds set-full's scan kernels and nothing else; set_full_host.hip
// (create, run, results) calls them.  Each takes the stream, the grid in workgroups of 256 and its kernel's own arguments.  The plan table
// goes over as const void*: SfKeyPlan, like everything in set_full_plan.h, is a type of the including unit (an unnamed namespace), and a
// function between two units cannot name it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// create: p[r], how many elements had been invoked when read r completed, and the chunks' extremes of it
void sf_launch_prefix(hipStream_t s, uint32_t grid, const void* plan, const uint32_t* first, uint32_t n_keys, const uint32_t* add_invoke,
                      const uint32_t* read_ok, uint32_t* P, uint32_t* pmax);
// create: the matrix from the reads' compact form
void sf_launch_rows(hipStream_t s, uint32_t grid, const void* plan, const uint32_t* first, uint32_t n_keys, uint32_t R_all, const uint32_t* top,
                    const unsigned long long* exc_off, const uint32_t* exc, uint32_t* M);
// run: pass 1, the chunk summaries
void sf_launch_any(hipStream_t s, uint32_t grid, const void* plan, const uint32_t* first, uint32_t n_keys, const uint32_t* M, const uint32_t* P,
                   const uint32_t* pmax, uint32_t* any_p, uint32_t* any_a, unsigned long long* words_loaded);
// run: pass 2, the three indices per element
void sf_launch_resolve(hipStream_t s, uint32_t grid, const void* plan, const uint32_t* first, uint32_t n_keys, const uint32_t* M, const uint32_t* P,
                       const uint32_t* read_invoke, const uint32_t* read_ok, const uint32_t* any_p, const uint32_t* any_a, const uint32_t* add_ok,
                       uint32_t* lp, uint32_t* la, uint32_t* known, unsigned long long* words_loaded);
