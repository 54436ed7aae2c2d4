/*
 * bisbm_io.h -- host-side text I/O of the engine, format-identical with the reference's
 * graph_utilities.cc / output_functions.hh (paths relative to /root/reference/src).  Part of
 * libbisbm_hip.so; plain C ABI.  Buffers returned through ** are malloc'ed: release them with
 * bisbm_io_free.
 */
#ifndef BISBM_IO_H
#define BISBM_IO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* load_edge_list (graph_utilities.cc:20-34): one "a b" pair per line, any blanks between.  Same
 * quirks as the stringstream loop: a blank line repeats the previous pair, a non-numeric line
 * gives (0, previous b), a single number keeps the previous b.  Returns the number of lines, or
 * -1 when the file cannot be opened. */
long bisbm_io_read_edge_list(const char *path, uint64_t **a, uint64_t **b);

/* load_memberships (graph_utilities.cc:5-18): one label per line.  Returns the count or -1. */
long bisbm_io_read_memberships(const char *path, uint32_t **labels);

/* The clamp file of `mcmc --clamp` (no reference counterpart; include/bisbm.h, "Clamped nodes"): node ids as decimal numbers
 * separated by white space (blanks, tabs, line ends), in any order, repeats allowed; an empty file is an empty clamp.  *mask
 * gets n malloc'ed bytes, 1 for every listed node.  Returns the number of distinct nodes listed, -1 when the file cannot be
 * opened, -2 for a token that is not a number of decimal digits alone (a sign, a letter) or an id >= n (a number past 2^64
 * included); `err` (err_cap bytes, may be NULL) then holds a message that names the token, and *mask is NULL. */
long bisbm_io_read_clamp(const char *path, uint64_t n, uint8_t **mask, char *err, size_t err_cap);

/* The constraints file of `mcmc --constraints` (no reference counterpart; include/bisbm.h, "Block constraints"): one line per
 * constrained node -- the node id, then its allowed blocks as global labels (type a: 0 .. ka-1, type b: ka .. ka+kb-1), all
 * decimal numbers separated by blanks or tabs.  Lines in any order; a node may be repeated with the same blocks; blank lines
 * are skipped; an empty file constrains nobody.  The lists become classes: class 0 allows everything and holds the unlisted
 * nodes, every distinct list (as a set, per type) gets the next class, at most 255 of them.  *class_of_node gets n malloc'ed
 * bytes and *allowed a malloc'ed table of classes x (ka + kb) bytes, 1 = allowed (the columns of the other type are 1: they
 * are ignored).  Returns the number of classes (>= 1), -1 when the file cannot be opened, -2 for a malformed line: a token
 * that is not a number of decimal digits alone, a node id >= n or a block >= ka + kb (a number past 2^64 included), a block of
 * the other type, a node without a block, a node repeated with other blocks, a 256th distinct list; `err` (err_cap bytes, may
 * be NULL) then holds a message that names the offending token, and both outputs are NULL. */
long bisbm_io_read_constraints(const char *path, uint64_t n, uint64_t na, uint32_t ka, uint32_t kb, uint8_t **class_of_node,
                               uint8_t **allowed, char *err, size_t err_cap);

/* The fields file of `mcmc --fields` (no reference counterpart; include/bisbm.h, "Block fields"): one line per node with a
 * prior -- the node id, then block:weight pairs, the block a global label of the node's type, the weight a finite decimal or
 * scientific number above 0; tokens separated by blanks or tabs.  The energy of a listed block is phi = -ln weight (the host
 * libm's log), an unlisted block has weight 1, phi = 0.  Lines in any order; a node may be repeated with the same row (a
 * repeat with another row is an error, not "the last line wins"); blank lines are skipped; an empty file gives nobody a field.
 * The rows become classes: class 0 is the zero row and holds the unlisted nodes, every distinct row gets the next class, at most
 * 255 of them.  *class_of_node gets n malloc'ed bytes and *field a malloc'ed table of classes x (ka + kb) doubles.  Returns the
 * number of classes (>= 1), -1 when the file cannot be opened, -2 for a malformed line: a node id or block that is not a number
 * of decimal digits alone, a node id >= n or a block >= ka + kb, a block of the other type, a block twice on a line, a token
 * without ':', a weight that is not a number, is 0 (the message names --constraints), negative or not finite, a node without a
 * pair, a node repeated with another row, a 256th distinct row; `err` (err_cap bytes, may be NULL) then holds a message that
 * names the offending token, and both outputs are NULL. */
long bisbm_io_read_fields(const char *path, uint64_t n, uint64_t na, uint32_t ka, uint32_t kb, uint8_t **class_of_node,
                          double **field, char *err, size_t err_cap);

/* edge_to_adj (graph_utilities.cc:36-49) as CSR: undirected, duplicates kept, each row in edge-file
 * order.  rowptr has n+1 entries, col has 2*n_edges.  Returns 0, or -1 when an id is >= n. */
int bisbm_io_edges_to_csr(const uint64_t *a, const uint64_t *b, size_t n_edges, uint64_t n,
                          uint64_t *rowptr, uint32_t *col);

/* load_edge_list + edge_to_adj in one call, with an optional binary cache beside the text file
 * (1e7..5e7-line edge lists through a line parser are slow; the TEXT FORMAT IS UNTOUCHED and stays the
 * source of truth).  The cache is `<path>.bisbm_csr`: a 48-byte header {magic "BISBMCSR", version, size and mtime
 * (ns) of the text file, n, n_edges}, then rowptr (n+1 x u64) and col (2 n_edges x u32) exactly as
 * bisbm_io_edges_to_csr builds them.  It is used only when size, mtime, n and the file's own length all match, and
 * rewritten (temporary file + rename) otherwise; a directory that cannot be written to just means no cache.
 * use_cache = 0: always parse the text, never touch a cache file.
 * Returns 0 and malloc'ed arrays (bisbm_io_free), -1 when the text file cannot be opened, -2 when an id is >= n.
 * *cache_hit (may be NULL) tells whether the arrays came from the cache. */
int bisbm_io_load_csr(const char *path, uint64_t n, int use_cache, uint64_t **rowptr, uint32_t **col,
                      uint64_t *n_edges, int *cache_hit);

/* Optional ingest-time renumbering for graphs whose node ids carry no structure.  The production
 * kernel visits ids in an id-local order and gathers the labels of their neighbours; that pays when nearby ids have
 * nearby neighbours.  This pass embeds both node types in a few dimensions (power iteration on the degree-normalised
 * bipartite adjacency, orthonormalised every round: the leading block structure), cuts the embedding with a median
 * kd-tree shared by both types, and numbers the nodes cell by cell.  new_id[v] is the new id of node v: a bijection
 * that keeps type-a nodes in [0, na) and type-b nodes in [na, n).  Deterministic.  Purely an optimisation of memory
 * locality: the engine run on the renumbered graph is a different (equally valid) chain, so this is never applied
 * behind the caller's back.  Returns 0, or -1 on bad arguments. */
int bisbm_io_locality_order(uint64_t n, uint64_t na, const uint64_t *rowptr, const uint32_t *col, uint32_t *new_id);

/* CSR of the renumbered graph: row new_id[v] = row v with every neighbour id mapped, order inside rows kept. */
int bisbm_io_permute_csr(uint64_t n, const uint64_t *rowptr, const uint32_t *col, const uint32_t *new_id,
                         uint64_t *rowptr_out, uint32_t *col_out);

/* output_vec (output_functions.hh:20-29): every element followed by one blank, then '\n'.
 * Returns the length written (without the NUL); call with out == NULL to size the buffer. */
size_t bisbm_io_format_labels(const uint32_t *labels, size_t n, char *out, size_t cap);

void bisbm_io_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
