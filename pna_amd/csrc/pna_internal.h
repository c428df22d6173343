// Internal helpers shared by the translation units of libpna_amd.so (not part of the C ABI).
#ifndef PNA_INTERNAL_H
#define PNA_INTERNAL_H
// Records `msg` as the calling thread's last error and returns `code`.
int pna_set_error(int code, const char* msg);
// PNA_E_INVALID with both sizes in the message when a caller's args struct is shorter than this library's (0 = fine).
int pna_check_struct_size(const char* fn, unsigned got, unsigned long need);
// PNA_E_INVALID with the message "<fn>: <clause>".
int pna_refuse(const char* fn, const char* clause);
// Lets `kernel` launch with `bytes` of dynamic LDS (an attribute is needed above 64 KiB); PNA_E_LAUNCH with the message `who` when the
// runtime refuses it.
int pna_raise_lds(const void* kernel, unsigned long bytes, const char* who);
// pna_segreduce_bwd_pull_f32 with one more operand for callers inside the library: `add` (n_src, ld_add) is added to the pulled rows
// in the ranked pull's store (a residual's gradient), NULL = the entry point itself.  The per-edge form (edge_rows) does not take it.
struct pna_segreduce_bwd_pull_args;
int pna_segreduce_bwd_pull_launch(const pna_segreduce_bwd_pull_args* q, const float* add, long ld_add, void* stream);
#endif
