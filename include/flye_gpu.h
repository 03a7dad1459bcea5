/* flye_gpu.h -- C ABI of the MI355X-native overlap hot path (libflyegpu.so).
 *
 * Drop-in boundary for the two seams of Flye 2.8.1's sequence library
 * (citations are into the reference tree):
 *
 *   index build        VertexIndex::countKmers / buildIndexUnevenCoverage /
 *                      buildIndexMinimizers / clear / getSampleRate
 *                      (src/sequence/vertex_index.h:213-218, :260;
 *                       src/sequence/vertex_index.cpp:19-125, :389-483)
 *   per-read overlaps  OverlapDetector::getSeqOverlaps, reached only through
 *                      OverlapContainer::quickSeqOverlaps / lazySeqOverlaps
 *                      (src/sequence/overlap.h:338-345, overlap.cpp:99-508,
 *                       :518-574)
 *
 * The reference has no FFI: these entry points are what a C++ binding inside
 * VertexIndex / OverlapContainer would call (see INTEGRATION.md for the stub).
 * Conventions: every call returns an int status (FG_OK = 0, < 0 = error, text
 * via fg_strerror); no exceptions cross the boundary; plain pointers + sizes;
 * a context is bound to one HIP device and may be used by one host thread at
 * a time.  There is NO CPU fallback: without a usable HIP device fg_create
 * fails with FG_ERR_NO_DEVICE.
 */
#ifndef FLYE_GPU_H
#define FLYE_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FG_ABI_VERSION 4

enum {
	FG_OK = 0,
	FG_ERR_NO_DEVICE = -1,   /* no HIP device / HIP runtime failure at create */
	FG_ERR_HIP = -2,         /* a HIP call failed; fg_last_error() has the text */
	FG_ERR_ARG = -3,         /* bad argument */
	FG_ERR_STATE = -4,       /* call order: reads not set / index not built */
	FG_ERR_KMER_TOO_FREQUENT = -5, /* vertex_index.cpp:372 "k-mer is too frequent" */
	FG_ERR_KMER_SIZE = -6,   /* k > 17 with the flat counter, vertex_index.cpp:504-507;
	                            k > 32 never fits Kmer::KmerRepr (kmer.h:19) */
	FG_ERR_UNSUPPORTED = -7, /* flag combination not built yet */
	FG_ERR_NOMEM = -8
};

typedef struct fg_ctx fg_ctx;

/* Parameters::get().kmerSize (src/common/config.h:103-115) is process-global
 * in the reference; here it is a property of the context.
 * The FIRST fg_create of a process initialises the HIP runtime, which draws from libc's rand() stream; the
 * call parks the caller's stream in a private state array for that time (initstate / setstate) so that the
 * reference's own rand() consumers (overlap.cpp:752-756, chimera.cpp:76, sequence_container.cpp:318-328) see
 * the numbers they would have seen.  That swap is process-wide: make the first fg_create from a thread
 * beside which no other thread calls rand() (Flye: the main thread, at index build).  Later calls swap nothing. */
int  fg_create(fg_ctx** out, int device, int kmer_size);
void fg_destroy(fg_ctx* ctx);
const char* fg_strerror(int code);
const char* fg_last_error(const fg_ctx* ctx);   /* NULL: the calling thread's last failed fg_paf_parse ("" before any) */
int  fg_abi_version(void);

/* Id range of the indexed container and of the optional query container (n_fwd forward records
 * each, ids first_id + 2i and their reverse complements + 1); any pointer may be NULL. */
int fg_container_info(const fg_ctx* ctx, uint32_t* first_id, uint32_t* n_fwd,
                      uint32_t* query_first_id, uint32_t* query_n_fwd);

/* SequenceContainer contents (src/sequence/sequence_container.cpp:48-79,
 * :359-392).  Forward strands only; the reverse complement of read i is
 * implied (FastaRecord::Id first_seq_id + 2i is the forward record, +1 its
 * reverse complement, sequence_container.h:27-33).  Packing is DnaSequence's
 * (src/sequence/sequence.h:54-69): 32 nt per uint64, nt j at bits (j%32)*2,
 * A,C,G,T = 0..3; each read starts on a word boundary; word_off has n+1
 * entries.  N-replacement (sequence_container.cpp:318-328) stays with the
 * caller because it draws from libc rand().  The buffers are copied to HBM;
 * the caller may free them on return. */
int fg_set_reads(fg_ctx* ctx, uint32_t n_fwd, const uint64_t* words,
                 const uint64_t* word_off, const int32_t* len,
                 uint32_t first_seq_id);

/* Optional second SequenceContainer holding the QUERIES, for callers whose queries are not
 * the indexed sequences: ReadAligner::alignReads indexes the graph edge sequences and
 * queries every read against them (src/repeat_graph/read_aligner.cpp:178-217).  Same
 * layout as fg_set_reads; the ids must not overlap the indexed container's (the reference
 * draws both from one process-wide counter, sequence_container.cpp:16, :55-60).  n_fwd = 0
 * returns to "queries are the indexed reads".  fg_set_reads() also resets it. */
int fg_set_queries(fg_ctx* ctx, uint32_t n_fwd, const uint64_t* words,
                   const uint64_t* word_off, const int32_t* len,
                   uint32_t first_seq_id);

struct fg_index_stats {
	uint64_t total_kmers;      /* KmerCounter::_numKmers: distinct canonical k-mers
	                              ("Total k-mers", vertex_index.cpp:589); 0 in
	                              minimizer mode */
	uint64_t selected_kmers;   /* _kmerIndex.size() ("Selected k-mers", :121, :473) */
	uint64_t index_entries;    /* "Index size" (:122) / "K-mer index size" (:474) */
	uint64_t repetitive_kmers; /* _repetitiveKmers.size() */
	uint64_t repetitive_frequency; /* _repetitiveFrequency (:186) */
	float    mean_frequency;   /* meanFrequency (:185) */
	float    sample_rate;      /* VertexIndex::getSampleRate(): ctor value, or
	                              totalLen/entries after buildIndexMinimizers (:480-482) */
	double   build_seconds;    /* device time of the build, HIP events */
};

/* countKmers() + buildIndexUnevenCoverage(min_freq, select_rate, tandem_freq)
 * with Config "repeat_kmer_rate" = repeat_rate (vertex_index.cpp:19-125,
 * :173-212, :316-358, :499-590).  sample_rate_init is the VertexIndex ctor
 * argument (main_assemble.cpp:195-196). */
int fg_build_index_solid(fg_ctx* ctx, int32_t min_freq, float select_rate,
                         int32_t tandem_freq, float repeat_rate,
                         float sample_rate_init, struct fg_index_stats* out);

/* buildIndexMinimizers(min_coverage, window) (vertex_index.cpp:389-483,
 * kmer.h:206-262). */
int fg_build_index_minimizers(fg_ctx* ctx, int32_t min_coverage, int32_t window,
                              float repeat_rate, struct fg_index_stats* out);

/* The same builds in steps, for sharding over GPUs and for bounded memory:
 *   begin        the k-mer selection over ALL reads of the container (it needs every read: exact counts,
 *                per-read frequency thresholds / minimizers); hist[FG_INDEX_BINS] receives the number of
 *                accepted k-mer positions per key bin (bin = canonical k-mer >> max(0, 2k - 12));
 *   build_range  sorts and run-length encodes the keys of bins [bin_lo, bin_hi) -- each rank its own
 *                range; sums[2] = this context's running share of filterFrequentKmers' two integer sums
 *                (vertex_index.cpp:175-184), to be added up over the ranks;
 *   finish       total_sums (NULL = this context's own) fix the repetitive frequency; the context then
 *                holds a usable index over the ranges it built (fg_export_index / fg_index_device_arrays
 *                give the pieces; the all-gathered concatenation goes into fg_import_index).
 * fg_build_index_solid / _minimizers = begin + build_range(0, FG_INDEX_BINS) + finish(NULL). */
#define FG_INDEX_BINS 4096
int fg_index_begin_solid(fg_ctx* ctx, int32_t min_freq, float select_rate, int32_t tandem_freq,
                         float repeat_rate, float sample_rate_init, uint64_t* hist);
int fg_index_begin_minimizers(fg_ctx* ctx, int32_t min_coverage, int32_t window, float repeat_rate,
                              uint64_t* hist);
int fg_index_build_range(fg_ctx* ctx, uint32_t bin_lo, uint32_t bin_hi, uint64_t* sums);
int fg_index_finish(fg_ctx* ctx, const uint64_t* total_sums, struct fg_index_stats* out);

/* The solid-mode selection in steps of its own: bounded memory on one GPU, and on several GPUs the exact counters
 * -- the 4^k * 4 B array that KmerCounter's flat array + overflow map become (vertex_index.cpp:499-616) -- held
 * only for a rank's own key range ("GPU g counts only canonical k-mers [of its slice] over all
 * reads"):
 *   kmer_hist       hist[FG_INDEX_BINS] = ALL k-mer positions per key bin: what the ranks' key ranges are balanced
 *                   on before anything is selected (the same ranges then serve fg_index_build_range);
 *   count_slice     allocates the counters of bins [bin_lo, bin_hi) and counts those k-mers over all reads;
 *                   *distinct = this range's share of "Total k-mers" (vertex_index.cpp:589; adds up over ranks);
 *                   *n_batches = the batches of reads the selection then runs in (<= FG_INDEX_BATCH_KMERS k-mer
 *                   positions each, default 2^28: the selection's scratch is bounded by that, not by the read set);
 *   batch_freq      KmerCounter::getFreq of every k-mer position of batch b as far as THIS context counted it (0
 *                   outside its range) into a device array (*d_freq, *n uint32): summed over the ranks in place
 *                   (all-reduce) it is the complete array; on one GPU it already is.  The array is complete when
 *                   the call returns; the caller's reduction must itself be COMPLETE (host-synchronised: the library
 *                   works on its own streams) before batch_select is called;
 *   batch_select    yieldFrequentKmers (vertex_index.cpp:316-358) over the batch's reads from that array;
 *   selection_done  releases the batch scratch; hist[] as fg_index_begin_solid gives it.
 * fg_index_begin_solid = count_slice(0, FG_INDEX_BINS) + {batch_freq, batch_select} per batch + selection_done.
 * fg_index_build_range then accepts only bins inside the counted range (the finish step asks the counters
 * about the keys it built, vertex_index.cpp:70-71). */
int fg_index_kmer_hist(fg_ctx* ctx, uint64_t* hist);
int fg_index_count_slice(fg_ctx* ctx, int32_t min_freq, float select_rate, int32_t tandem_freq, float repeat_rate,
                         float sample_rate_init, uint32_t bin_lo, uint32_t bin_hi, uint64_t* distinct,
                         uint32_t* n_batches);
int fg_index_batch_freq(fg_ctx* ctx, uint32_t batch, uint32_t** d_freq, uint64_t* n);
int fg_index_batch_select(fg_ctx* ctx, uint32_t batch);
int fg_index_selection_done(fg_ctx* ctx, uint64_t* hist);

/* The all-gather of a sharded build without a second copy of the index.  After fg_index_finish the context holds
 * its own piece.  gather_begin sets that piece aside and makes the context's arrays the full-size ones
 * (n_keys, n_entries, n_repetitive = the totals over the ranks); full[4] / piece[4] receive the DEVICE pointers
 * of {keys, key_off (n_keys + 1), entries, repetitive keys} of the full arrays and of the own piece,
 * piece_sizes[3] = {keys, entries, repetitive} of the piece.  The caller's collective writes every rank's piece
 * -- the own one included, list offsets shifted by the entries of the pieces before -- straight into the full
 * arrays; gather_end frees the piece, checks the arrays (FG_ERR_ARG when offsets or keys are out of order) and
 * builds the lookup structures. */
int fg_index_gather_begin(fg_ctx* ctx, uint64_t n_keys, uint64_t n_entries, uint64_t n_repetitive,
                          uint64_t** full, uint64_t** piece, uint64_t* piece_sizes);
int fg_index_gather_end(fg_ctx* ctx, float sample_rate);

/* Device bytes this library holds right now and at most since the last reset (all contexts of the process;
 * every device allocation of the library is counted); reset_peak != 0 restarts the peak at the current value. */
int fg_memory_stats(uint64_t* bytes_now, uint64_t* bytes_peak, int reset_peak);

/* An index given as CSR arrays in the layout fg_export_index writes (keys ascending, key_off[n_keys + 1],
 * entries ascending per key), in host memory or -- on_device != 0 -- in this context's device memory
 * (e.g. torch tensors filled by an RCCL all-gather).  sample_rate = VertexIndex::getSampleRate().
 * The arrays are checked on the device (offsets start at 0, never decrease, end at n_entries; keys strictly
 * ascending): FG_ERR_ARG otherwise. */
int fg_import_index(fg_ctx* ctx, uint64_t n_keys, const uint64_t* keys, const uint64_t* key_off,
                    uint64_t n_entries, const uint64_t* entries, uint64_t n_repetitive,
                    const uint64_t* repetitive_keys, float sample_rate, int on_device);

/* Device pointers of the built index (valid until the next build / import / clear), for collectives
 * that run on device memory. */
int fg_index_device_arrays(fg_ctx* ctx, uint64_t* n_keys, uint64_t* n_entries, uint64_t* n_repetitive,
                           const uint64_t** keys, const uint64_t** key_off, const uint64_t** entries,
                           const uint64_t** repetitive_keys);

/* VertexIndex::clear() (vertex_index.cpp:486-496) */
int fg_clear_index(fg_ctx* ctx);


/* Read-only export of the built index for parity tests: keys ascending,
 * key_off[n_keys+1] into entries; an entry is (record_index << 32) | position
 * with record_index = FastaRecord id - first_seq_id, i.e. the same order as the
 * reference's global position (vertex_index.cpp:108-114).  Pass NULL pointers
 * to query the sizes. */
int fg_export_index(fg_ctx* ctx, uint64_t* n_keys, uint64_t* n_entries,
                    uint64_t* n_repetitive, uint64_t* keys, uint64_t* key_off,
                    uint64_t* entries, uint64_t* repetitive_keys);

/* OverlapDetector constructor arguments (overlap.h:313-336) */
struct fg_detector_params {
	int32_t max_jump;
	int32_t min_overlap;
	int32_t max_overhang;          /* 0 => _checkOverhang = false */
	uint8_t keep_alignment;        /* 1: also return every overlap's kmerMatches (the chain thinned
	                                  to one match per > k query bases, overlap.cpp:368-377,
	                                  398-405) in fg_overlap_batch.matches */
	uint8_t only_max_ext;          /* 1: best overlap per target (assemble); 0: all primaries
	                                  not contained in a better one (overlap.cpp:441-458) */
	uint8_t nucl_alignment;        /* base-level divergence (alignment.cpp:218-247) */
	uint8_t partition_bad_mappings;/* 1: primaries that FAIL the divergence gate are returned too,
	                                  marked in fg_overlap_batch.needs_trim, in the position
	                                  where the caller splices in the pieces checkIdyAndTrim
	                                  keeps (overlap.cpp:474-485): fg_trim_ranges computes them
	                                  on the device for these records.  Only with max_overlaps = 0, as every
	                                  caller in the reference uses it (overlap.h:323);
	                                  FG_ERR_UNSUPPORTED otherwise */
	uint8_t use_hpc;
	uint8_t pad_[3];
	float   max_divergence;        /* OverlapDetector::_maxDivergence (mutable,
	                                  set by setDivergenceThreshold, overlap.cpp:820-827) */
};

/* One OverlapRange (overlap.h:20-279) plus the integers the float was made of.
 * seq_divergence is computed on the HOST with glibc logf/float division from the
 * device integers, exactly as overlap.cpp:417-423 / alignment.cpp:244-245 do. */
struct fg_overlap_rec {
	uint32_t cur_id, ext_id;
	int32_t  cur_begin, cur_end, cur_len;
	int32_t  ext_begin, ext_end, ext_len;
	int32_t  score;
	float    seq_divergence;
	int32_t  chain_length;        /* chainLength (overlap.cpp:366) */
	int32_t  filtered_positions;  /* repetitive query positions in range (:407-413) */
	int32_t  edit_distance;       /* -1 unless nucl_alignment */
	int32_t  hpc_len_cur, hpc_len_ext; /* compared string lengths (after HPC if on) */
};

struct fg_overlap_batch {
	uint32_t n_queries;
	uint64_t n_recs;
	uint64_t* query_off;           /* n_queries + 1, into recs */
	struct fg_overlap_rec* recs;   /* per query: reference emission order
	                                  (ascending ext_id, overlap.cpp:216-234) */
	uint64_t n_div_stats;
	uint64_t* div_stats_off;       /* n_queries + 1 */
	float*   div_stats;            /* OvlpDivStats::add() values (:488-506) */
	/* keep_alignment only (else 0 / NULL): OverlapRange::kmerMatches of recs[i] is the
	 * (cur, ext) int32 pairs matches[2*match_off[i]] .. matches[2*match_off[i+1]-1] */
	uint64_t n_matches;            /* pairs in total */
	uint64_t* match_off;           /* n_recs + 1 */
	int32_t* matches;
	/* partition_bad_mappings only (else NULL): needs_trim[i] = 1 when recs[i] did not pass
	 * seq_divergence < max_divergence and is there for the caller's checkIdyAndTrim */
	uint8_t* needs_trim;           /* n_recs */
	/* work counters of this call (for the roofline's m and d) */
	uint64_t query_bp, query_kmers, seed_hits, dp_groups, dp_elements;
	uint64_t dp_elements_small;    /* of dp_elements: in the groups the one-kernel chaining path takes: <= 256 hits
	                                * before the prefilter by default, <= FG_FUSED_CAP with that switch, none with
	                                * FG_CHAIN_FUSED=0 */
	double   device_seconds;       /* HIP-event time of the whole call */
	void*    owner_;               /* library arena; release with fg_release_batch */
};

/* getSeqOverlaps for a batch of FastaRecord ids (forward or reverse-complement
 * ids), as OverlapContainer::quickSeqOverlaps(id, max_overlaps, force_local)
 * would return them one by one (overlap.cpp:518-526). */
int fg_overlaps(fg_ctx* ctx, const struct fg_detector_params* p,
                const uint32_t* query_ids, uint32_t n_queries,
                int32_t max_overlaps, uint8_t force_local,
                struct fg_overlap_batch* out);
void fg_release_batch(struct fg_overlap_batch* b);

/* Option B of the multi-GPU layout: the index sharded by TARGET read.  Every rank keeps the list
 * entries of the target reads it owns, probes ALL queries against that shard (fg_probe_hits) and sends each query's
 * seed hits to the query's owner, which restores the reference's emission order and runs the rest of getSeqOverlaps
 * on them (fg_overlaps_from_hits).
 *
 * fg_index_keep_targets restricts a complete index (a build, an option-A gather or an import) to the entries whose
 * target read index i = (record id - first_seq_id) >> 1 has i % world == rank.  Each key's list stays ascending, the
 * entry array shrinks to the kept entries (the memory goes back to the device).  Keys, the lookup table, the
 * repetitive k-mers and getSampleRate() are kept as they are: minimizer mode takes the sample rate over the WHOLE
 * index (vertex_index.cpp:480-482), and it feeds the divergence estimate (overlap.cpp:420).  A restricted context
 * refuses fg_overlaps and fgb_create (FG_ERR_STATE): its lists hold 1/world of the targets.  A new build, an import
 * or fg_clear_index lifts the restriction.  world == 1 changes nothing; rank >= world is FG_ERR_ARG; no index is
 * FG_ERR_STATE; a second restriction to another (world, rank) is FG_ERR_STATE.  *n_entries_kept may be NULL.
 * fg_index_shard reports the restriction (world = 1, rank = 0 when there is none). */
int fg_index_keep_targets(fg_ctx* ctx, uint32_t world, uint32_t rank, uint64_t* n_entries_kept);
int fg_index_shard(const fg_ctx* ctx, uint32_t* world, uint32_t* rank);

/* The same shard built DIRECTLY from the key-range pieces of a sharded build, without any rank ever holding the full
 * entry array.  Rank order is key order; an entry's owner is ((entry >> 33) % world), as in fg_index_keep_targets.
 *
 * fg_index_piece_split, after fg_index_finish on a context that holds a piece (or a whole index): *d_counts receives
 * the device pointer of the world x n_keys matrix (uint64, row d contiguous) of "entries of key j owned by rank d",
 * *d_entries that of the piece's n_entries entries rewritten destination major, key major inside a destination, list
 * order inside a key (a stable world-way partition of every list); dest_totals[world] (host) = entries per
 * destination.  The piece itself is untouched.  The two buffers belong to the context and live until
 * fg_index_scatter_end, a new build, an import or fg_clear_index.  world == 0 or world > 128 is FG_ERR_ARG; no
 * finished piece, a gather or scatter in progress, or an already restricted context is FG_ERR_STATE.
 *
 * fg_index_scatter_begin (after a split for the same world) sets the piece and its split buffers aside -- the
 * pointers fg_index_device_arrays gave for the piece stay valid until scatter_end -- and allocates the shard's arrays:
 * full[4] = device pointers of keys[n_keys], key_off[n_keys + 1], entries[n_shard_entries],
 * repetitive[n_repetitive].  The caller's collectives fill them: keys and repetitive keys of all pieces in rank
 * order; into key_off[0 .. n_keys) the COUNT rows received from the sources in rank order (source s sends its row
 * `rank`); into entries the sources' segments for `rank`, in rank order.  rank >= world or world == 0 is FG_ERR_ARG.
 *
 * fg_index_scatter_end frees the piece and the split buffers, turns the counts into list offsets (exclusive scan in
 * place) and checks on the device, before any list is read through them: offsets end at n_shard_entries, keys
 * strictly ascending, every entry owned by `rank`, every list strictly ascending.  A violation is FG_ERR_ARG and
 * leaves the context without an index.  Then the lookup structures are built and the context is a shard exactly as
 * after fg_index_keep_targets(world, rank): fg_index_shard, the refusals of fg_overlaps / fgb_create, fg_probe_hits
 * and fg_overlaps_from_hits.  sample_rate = getSampleRate() of the WHOLE index. */
int fg_index_piece_split(fg_ctx* ctx, uint32_t world, const uint64_t** d_counts, const uint64_t** d_entries,
                         uint64_t* dest_totals);
int fg_index_scatter_begin(fg_ctx* ctx, uint32_t world, uint32_t rank, uint64_t n_keys, uint64_t n_shard_entries,
                           uint64_t n_repetitive, uint64_t** full);
int fg_index_scatter_end(fg_ctx* ctx, float sample_rate);

/* One seed hit as getSeqOverlaps collects it (overlap.cpp:176-196): KmerMatch{curPos, extPos, extId}, the target
 * side in the query k-mer's orientation (vertex_index.h:158-174). */
struct fg_seed_hit { int32_t cur_pos; int32_t ext_pos; uint32_t ext_id; };

/* Seed collection only, against this context's (shard) index: hit_counts[q] per query to the host; the hits in
 * device memory owned by the context (*d_hits, *n_hits in total; valid until the next call on the context), query
 * after query in list order, each query's in emission order (ascending curPos, then ascending stored global
 * position; the trivial self hit dropped, overlap.cpp:188-190).  Queries live in the container fg_set_queries gave,
 * if any.  FG_ERR_NOMEM when the hits do not fit the device. */
int fg_probe_hits(fg_ctx* ctx, const uint32_t* query_ids, uint32_t n_queries, uint64_t* hit_counts,
                  const struct fg_seed_hit** d_hits, uint64_t* n_hits);

/* getSeqOverlaps for query_ids, as fg_overlaps returns it on the FULL index, from the seed hits that n_src index
 * shards (fg_probe_hits) produced for them.  d_hits (device memory of this context's device) holds the sources one
 * after another and, inside source s, the queries in list order, hit_counts[s * n_queries + q] hits each; the order
 * of the hits inside one (source, query) run is arbitrary.  The receiver restores the reference's emission order
 * (curPos, stored record, stored position) on the device; this context's own index supplies the repetitive query
 * positions (overlap.cpp:407-413) and must hold the same keys and repetitive k-mers as the shards (any shard of the
 * same index, or the full index).  FG_ERR_ARG for a hit outside its query or target. */
int fg_overlaps_from_hits(fg_ctx* ctx, const struct fg_detector_params* p, const uint32_t* query_ids,
                          uint32_t n_queries, int32_t max_overlaps, uint8_t force_local, uint32_t n_src,
                          const uint64_t* hit_counts, const struct fg_seed_hit* d_hits,
                          struct fg_overlap_batch* out);

/* A DEVICE GROUP: several contexts of ONE process, possibly on different devices, behind one handle -- option B for a
 * caller that is one multi-threaded process (Flye) and has no process group.  devices[i] is the HIP device of member
 * i; a device may be named more than once (its members then share the chip).  A group of two or more members runs one
 * host thread of its own per member, and a member is only ever touched by its thread (the caller's current device is
 * left alone); a group of one member runs on the caller's thread and, like the plain fg_* calls, makes the member's
 * device current there.  Between group calls fg_group_member(i) lends member i
 * to the caller for the read-only calls of this header (fg_kernel_times, fg_index_shard, fg_export_index, ...).
 * n_members == 0 or > 128 (the limit of fg_index_piece_split) is FG_ERR_ARG.  A group call that fails on a member
 * returns that member's code, and fg_group_last_error names the member and carries its text.  The first
 * fg_group_create of a process is subject to the note at fg_create.
 *
 * A group of ONE member is the plain context: fg_build_index_* and fg_overlaps, no split, no exchange.
 *
 * set_reads / set_queries give every member the same containers (replicated, as the one-process-per-GPU path does).
 *
 * fg_group_build_index_*: the index sharded by target read (member r keeps the entries of the reads i with
 * i % n_members == r, exactly the shard of fg_index_keep_targets(n_members, r)), built directly from key-range pieces:
 * key ranges balanced on fg_index_kmer_hist (solid) / the accepted positions (minimizers), per member count_slice,
 * per batch of reads {batch_freq, the frequencies summed over the members, batch_select}, build_range, the two sums
 * added up, finish, piece_split, scatter_begin, the pieces copied member to member (hipMemcpyPeerAsync), scatter_end.
 * The frequency sum moves every member's share of the array through a staging buffer of at most FG_GROUP_STAGE_BYTES
 * (environment, default 1 GiB) on the receiving member and adds it there (the one kernel of the group); then the
 * complete shares are copied back.  No member maps another member's memory.  *out = the statistics of the WHOLE
 * index, field for field what fg_build_index_* gives on one context (build_seconds: wall time of the call).
 * fg_group_build_info: how the last build ran.
 *
 * fg_group_overlaps = fg_overlaps on the full index, field for field, counters included (device_seconds: the largest
 * sum over a member of the kernel time of its fg_probe_hits calls and the device_seconds of its
 * fg_overlaps_from_hits calls; the member-to-member copies between the two are NOT in it, their wall time is
 * fg_group_stats.exchange_seconds).  The list is cut into batches of FG_GROUP_BATCH_READS queries
 * (environment, default 4096); inside a batch the queries are listed grouped by owner (read i -> member
 * i % n_members, both strands), caller's order inside an owner; every member probes that list against its shard
 * (fg_probe_hits), so its hits for one owner are one contiguous segment; the segments go, sources in member order,
 * into a receive buffer of the owner (grow-only, counted by fg_memory_stats), and the owner runs
 * fg_overlaps_from_hits.  The result comes back in the CALLER's query order; release it with fg_release_batch.
 * Before a build (or after fg_group_clear_index) every query call is FG_ERR_STATE. */
typedef struct fg_group fg_group;
int  fg_group_create(fg_group** out, const int* devices, uint32_t n_members, int kmer_size);
void fg_group_destroy(fg_group* g);
int  fg_group_size(const fg_group* g, uint32_t* n_members);
fg_ctx* fg_group_member(fg_group* g, uint32_t i);   /* borrowed; NULL when i is out of range */
const char* fg_group_last_error(const fg_group* g);
int fg_group_set_reads(fg_group* g, uint32_t n_fwd, const uint64_t* words, const uint64_t* word_off,
                       const int32_t* len, uint32_t first_seq_id);
int fg_group_set_queries(fg_group* g, uint32_t n_fwd, const uint64_t* words, const uint64_t* word_off,
                         const int32_t* len, uint32_t first_seq_id);
int fg_group_build_index_solid(fg_group* g, int32_t min_freq, float select_rate, int32_t tandem_freq,
                               float repeat_rate, float sample_rate_init, struct fg_index_stats* out);
int fg_group_build_index_minimizers(fg_group* g, int32_t min_coverage, int32_t window, float repeat_rate,
                                    struct fg_index_stats* out);
int fg_group_clear_index(fg_group* g);
int fg_group_overlaps(fg_group* g, const struct fg_detector_params* p, const uint32_t* query_ids,
                      uint32_t n_queries, int32_t max_overlaps, uint8_t force_local,
                      struct fg_overlap_batch* out);
/* of the last fg_group_overlaps: bytes of seed hits copied to a member other than the one that produced them, seed
 * hits in total, member-to-member copies issued (own segments included), wall time of the copies (per batch the
 * slowest member's, added up) */
struct fg_group_stats { uint64_t hits_moved_bytes, hits_total, peer_copies; double exchange_seconds; };
int fg_group_stats(const fg_group* g, struct fg_group_stats* out);
/* of the last fg_group_build_index_*: batches of reads of the solid selection (0 in minimizer mode), pieces that
 * went through the staging buffers in total and the most that one member took from one other member in one batch,
 * bytes the frequency sum and the scatter copied between members */
struct fg_group_build_info {
	uint32_t selection_batches, stage_pieces_max;
	uint64_t stage_pieces, freq_bytes, scatter_bytes;
};
int fg_group_build_info(const fg_group* g, struct fg_group_build_info* out);

/* Per-kernel device time of the most recent fg_overlaps / build call, measured
 * with hipEvents on the library's own stream.  names[i] are static strings. */
struct fg_kernel_time { const char* name; double seconds; uint64_t launches; };
int fg_kernel_times(fg_ctx* ctx, struct fg_kernel_time* out, int max_entries);

/* Test hook: run the device hit-sort kernel (std::sort order by key, ties as GCC
 * libstdc++ introsort leaves them) on n_seg independent segments of (key, val)
 * pairs, in place in the caller's host arrays; seg_off has n_seg + 1 entries. */
int fg_debug_sort_pairs(fg_ctx* ctx, uint64_t* keys, uint32_t* vals,
                        const uint64_t* seg_off, uint32_t n_seg);

/* Test hook: fg_debug_sort_pairs in the overlap stage's 64-bit key + value form (sequences of 2^24 bases and more, or
 * FG_PACKED_KEYS=0): key = ext_id << 32 | cur_pos with cur_pos < 2^cur_bits, and the sort is told cur_bits (0..32) as
 * the stage tells it.  cur_bits = 0 is fg_debug_sort_pairs. */
int fg_debug_sort_pairs64(fg_ctx* ctx, uint64_t* keys, uint32_t* vals, const uint64_t* seg_off, uint32_t n_seg,
                          int cur_bits);

/* Test hook: the same sort on the overlap stage's packed records, one 64-bit word per hit: record << (cur_bits + 24) |
 * cur_pos << 24 | ext_pos, ordered on word >> 24 alone (the low 24 bits travel as the value); no value array, no
 * tie-free flags, as the stage calls it.  cur_bits >= 0 and cur_bits + 24 < 64. */
int fg_debug_sort_packed(fg_ctx* ctx, uint64_t* recs, const uint64_t* seg_off, uint32_t n_seg, int cur_bits);

/* Test hook: the same sort in the overlap stage's 32-bit key form, key = record << cur_bits | cur_pos with rec_bits
 * record bits (cur_bits + rec_bits <= 32), every segment given by ascending cur_pos as the seed expansion emits it.
 * tie_free (n_seg words, or NULL = none): non-zero promises that the segment holds no two equal keys; such segments
 * of a middle size are sorted by stable radix passes over the record bits instead of the introsort emulation
 * (FG_SORT_TIEFREE=0 ignores the flags).  radix_segments / radix_hits: what took that path. */
int fg_debug_sort_pairs32(fg_ctx* ctx, uint32_t* keys, uint32_t* vals, const uint64_t* seg_off, uint32_t n_seg,
                          int cur_bits, int rec_bits, const uint32_t* tie_free,
                          uint64_t* radix_segments, uint64_t* radix_hits);

/* Test hook: fg_debug_sort_pairs32 with 16-bit values, the hit form the overlap stage takes when every target position
 * fits 16 bits (32-bit keys and an indexed container whose longest read has at most 65536 bases; FG_VAL16=0 keeps
 * 32-bit values).  vals are the caller's, sorted along with the keys. */
int fg_debug_sort_pairs32_val16(fg_ctx* ctx, uint32_t* keys, uint16_t* vals, const uint64_t* seg_off, uint32_t n_seg,
                                int cur_bits, int rec_bits, const uint32_t* tie_free,
                                uint64_t* radix_segments, uint64_t* radix_hits);

/* Test hook: *val16 = 1 when the last sub-range of queries this context expanded in an fg_overlaps call carried its
 * target positions as 16-bit values, else 0. */
int fg_debug_hit_val16(fg_ctx* ctx, uint32_t* val16);

/* Test hook: the per-query tie-free flags the seed expansion wrote for the last sub-range of queries this context
 * expanded in an fg_overlaps call (the whole call where it was not cut; none on the option-B receiver path and for
 * 64-bit key forms): *first_query = index of its first query in the call's query list, *n = its queries, out[i]
 * (i < min(max_n, *n)) = 1 when no two seed hits of query *first_query + i share (ext_id, cur_pos). */
int fg_debug_tie_free(fg_ctx* ctx, uint32_t* out, uint32_t max_n, uint32_t* first_query, uint32_t* n);

/* Test hook: the hit sort's screen for queries whose tied keys all lie in target groups the chaining prefilter drops, on
 * the caller's segments (keys as for fg_debug_sort_pairs32, every segment by ascending cur_pos, equal keys neighbours;
 * tie_free: n_seg words as k_fill writes them).  min_unique / min_overlap: the prefilter's bounds on a group's distinct
 * query positions (compared as float) and on its query span.  out_reason[i]: 0 = not screened (flagged tie-free, a size
 * the radix path does not take, or the screen is off: FG_SORT_SCREEN=0, FG_SORT_TIEFREE=0, cur_bits == 0), 1 = order-
 * free (no tied group can pass both bounds: any sort gives the same overlaps), 2 = a tied group may pass them, 3 =
 * more than 256 tied records. */
int fg_debug_sort_screen(fg_ctx* ctx, const uint32_t* keys, const uint64_t* seg_off, uint32_t n_seg, int cur_bits,
                         int rec_bits, const uint32_t* tie_free, float min_unique, int32_t min_overlap,
                         uint32_t* out_reason);

/* Test hook: the screen's reason words for the queries fg_debug_tie_free speaks of (same *first_query; *n = 0 where the
 * screen did not run). */
int fg_debug_order_free(fg_ctx* ctx, uint32_t* out_reason, uint32_t max_n, uint32_t* first_query, uint32_t* n);

/* Test hook: the number of segments the last hit sort of this context (the last sub-range of an fg_overlaps call, or a
 * fg_debug_sort_pairs* call) sent to the radix path. */
int fg_debug_sort_radix_segments(fg_ctx* ctx, uint32_t* segments);

/* Test hook (host only): the key ranges a group build of `world` members cuts from hist[FG_INDEX_BINS]; member r
 * gets the bins [cuts[r], cuts[r + 1]); cuts has world + 1 entries.  They equal dist.balanced_bin_ranges. */
int fg_debug_group_bin_cuts(const uint64_t* hist, uint32_t world, uint32_t* cuts);

/* Test hook: dst[i] += src[i] (uint32, wrapping) over n elements of the caller's host arrays through the device kernel
 * of the group's frequency sum (k_freq_accumulate).  The device copies keep each pointer's offset inside its 16 bytes:
 * an array that starts off a 16-byte boundary takes the kernel's unaligned path. */
int fg_debug_freq_accumulate(fg_ctx* ctx, uint32_t* dst, const uint32_t* src, uint64_t n);

/* Test hook: the device-wide prefix sum of the index build (fgprim::scan) over n elements of elem_bytes (4 or 8) bytes
 * in the caller's host array, in place: data[i] becomes the sum of data[0 .. i), or of data[0 .. i] when inclusive;
 * sums are modulo 2^(8 elem_bytes).  in_place != 0 runs the device scan with its output on its input, as the index
 * build does; otherwise on separate buffers.  Every device buffer has exactly the size the primitive is promised (the
 * scratch what its size function says) with a guard region behind it: a write past one is an FG_ERR_HIP.
 * n <= 2^40. */
int fg_debug_scan(fg_ctx* ctx, void* data, uint64_t n, int elem_bytes, int inclusive, int in_place);

/* Test hook: the stable radix sort of the index build and of the seed-hit exchange (fgprim::radixSortPairs) on n
 * (key, value) pairs of the caller's host arrays, in place: ordered by bits [begin_bit, end_bit) of the key alone,
 * pairs equal in those bits in their input order.  0 <= begin_bit <= end_bit <= 64, n <= 2^30 - 1; an empty bit
 * range leaves the arrays as they are.  passes_run (may be null): the 8-bit passes launched -- a pass in which every
 * key has the same digit is skipped.  Buffers are guarded as for fg_debug_scan. */
int fg_debug_radix_sort_pairs(fg_ctx* ctx, uint64_t* keys, uint64_t* vals, uint64_t n, int begin_bit, int end_bit,
                              int* passes_run);

/* Test hook for the probe skip of the overlap stage: one pass over the forward k-mer positions of all indexed reads.
 * A solid-k-mer build leaves one bit per position, "the k-mer's frequency over the whole read set reached min_freq";
 * where it is clear the seed collection takes the position for a miss without looking the k-mer up (a key enters the
 * index only through a position with that frequency).  In a build in steps the bits are taken from the arrays
 * fg_index_batch_select reads, which the caller has made complete over the ranks.  clear_bits: positions whose bit is
 * clear; violations: those among them whose k-mer does have a slot in the context's lookup table -- always 0.  Both
 * are 0 where the context holds no such bits (minimizer index, imported index, after fg_index_piece_split): every
 * k-mer is then looked up.  The environment switch FG_PROBE_SKIP=0 makes the overlap stage ignore the bits. */
int fg_debug_probe_skip_check(fg_ctx* ctx, uint64_t* clear_bits, uint64_t* violations);

/* Test hook (read only): the k-mer lookup table of the context's index as the kernels see it.  *wide = 1 for the
 * {key, key index} pair form (k >= 18), 0 for the one-word form (key << 30 | key index inside the part, all ones in
 * the index bits = a repetitive k-mer); *n_parts = key-range parts (at most FG_DEBUG_TABLE_MAX_PARTS); *n_slots =
 * slots over all parts.  Part p holds the keys in [bound[p], bound[p + 1]) (bound: *n_parts + 1 values) in groups[p]
 * 8-slot groups that start at slot slot_base[p]; the index a one-word slot stores counts from key key_base[p] of the
 * sorted key array.  slots: a copy of the slot array, *n_slots words, or 2 * *n_slots for the pair form (key, then key
 * index or all ones for a repetitive k-mer); an empty slot is all ones.  Every output pointer may be null: a call
 * with null arrays asks for the sizes.  FG_ERR_STATE without an index. */
#define FG_DEBUG_TABLE_MAX_PARTS 16
int fg_debug_table(fg_ctx* ctx, uint32_t* wide, uint32_t* n_parts, uint64_t* n_slots, uint64_t* bound,
                   uint64_t* slot_base, uint64_t* key_base, uint32_t* groups, uint64_t* slots);

/* Test hook for the lazy primary of the chaining stage (only_max_ext): how the groups of the last fg_overlaps call on
 * this context left the backtracking stage.  out[0]: groups that reached it (through the prefilter and the DP);
 * out[1]: groups whose primary was taken straight from the DP tables -- the live element of the strictly largest
 * score, its chain read once, no score order and no consuming walks; out[2]: groups without any chain start (no
 * candidate); out[3..5]: groups that took the full path because the top score was tied, because an element points at
 * element 0 while the best chain is rooted elsewhere, or because the best chain failed overlapTest.  With
 * only_max_ext = 0, or with the environment switch FG_CHAIN_LAZY=0, out[1..5] are 0.  All 0 before the first call. */
int fg_debug_chain_lazy(fg_ctx* ctx, uint64_t out[6]);

/* Test hook: the exact global edit distance (what edlibAlign(NW, TASK_DISTANCE, k = -1) returns,
 * reference src/sequence/alignment.cpp:233-238, src/sequence/edlib.cpp:141-296) of n_pairs string
 * pairs through the device kernels of the base-level divergence step.  Pair i = the forward
 * strands of reads 2i (rows) and 2i+1 (columns) of the container given to fg_set_reads;
 * use_hpc != 0 compresses homopolymers first (alignment.cpp:52-70).  out_len_a / out_len_b
 * receive the (compressed) lengths. */
int fg_debug_edit_distances(fg_ctx* ctx, uint32_t n_pairs, int use_hpc, int32_t* out_dist,
                            int32_t* out_len_a, int32_t* out_len_b);

/* getAlignmentCigarKsw (src/sequence/alignment.cpp:102-216) for a batch of (target, query)
 * string pairs: banded affine-gap global alignment (ksw_extz2 of the reference's lib/minimap2 with match 2,
 * mismatch -4, gap open 4, gap extend 2; band 64 doubling while too narrow; global backtrack) with the CIGAR
 * decoded into runs of '=', 'X', 'I', 'D' and the error rate (mismatches + indel bases) / max(length).
 * trg / qry: one byte per base (0..3), pair i at [off[i], off[i + 1]).  The DP and the backtrack run on the
 * device; the decoding of the M runs and the float on the host.  Runs of pair i: ops / lens[run_off[i] ..
 * run_off[i + 1]). */
struct fg_cigar_batch {
	uint32_t  n_pairs;
	uint64_t* run_off;
	uint8_t*  ops;        /* '=', 'X', 'I', 'D' */
	int32_t*  lens;
	float*    err_rate;   /* n_pairs */
	void*     owner_;
};
int fg_align_cigar_ksw(fg_ctx* ctx, uint32_t n_pairs, const uint8_t* trg, const uint64_t* trg_off,
                       const uint8_t* qry, const uint64_t* qry_off, struct fg_cigar_batch* out);
void fg_release_cigars(struct fg_cigar_batch* b);

/* The same alignment for ranges of the sequences that are resident on the device: the first half of checkIdyAndTrim
 * (alignment.cpp:306-495) for the records fg_overlaps marks in needs_trim.  Pair i: target = [cur_begin, cur_end) of
 * sequence cur_id, query = [ext_begin, ext_end) of sequence ext_id (the roles of alignment.cpp:319-321).  Ids are
 * FastaRecord ids (odd = reverse-complement strand); cur_id names a sequence of the fg_set_queries container when one
 * is set, otherwise of the indexed container; ext_id always one of the indexed container.  use_hpc != 0: both strings
 * go through homopolymerCompression (alignment.cpp:52-70) first.  out (released with fg_release_cigars) equals, field
 * for field, what fg_align_cigar_ksw returns for those byte strings; len_cur / len_ext (may be NULL) receive the
 * aligned (compressed) lengths.  The strings are cut out of the 2-bit reads, aligned and decoded on the device: no
 * string crosses the bus.  Empty ranges are legal and behave as empty strings do.  FG_ERR_STATE without reads;
 * FG_ERR_ARG for an unknown id, begin < 0, end < begin, end > length, or NULL pairs / out with n_pairs > 0 -- found
 * before any device work.  The second half of checkIdyAndTrim is fg_trim_ranges below. */
struct fg_range_pair { uint32_t cur_id, ext_id; int32_t cur_begin, cur_end, ext_begin, ext_end; };
int fg_align_ranges(fg_ctx* ctx, const struct fg_range_pair* pairs, uint32_t n_pairs, uint8_t use_hpc,
                    struct fg_cigar_batch* out, int32_t* len_cur, int32_t* len_ext);

/* checkIdyAndTrim (alignment.cpp:306-495) as a whole for the same pairs: the alignment of fg_align_ranges, then, on the
 * runs while they are on the device, the search for the intervals of runs that begin and end on a '=' run with
 * float(errors) / max(cur span, ext span) < max_divergence (:366-385), their std::sort by that length (:389; the
 * permutation libstdc++ produces, ties included), the greedy non-intersecting selection (:393-409), the mapping back
 * through the homopolymer offset tables and the filter "both ranges > min_overlap" (:414-456).  No run list crosses
 * the bus.  Records of pair i: recs[rec_off[i] .. rec_off[i + 1]) in the order checkIdyAndTrim returns them.
 * cur_end / ext_end are what the reference leaves there: begin of the pair's range + the offset of the LAST aligned
 * base (:444-445), not one past it.  run_start / run_end: the chosen interval, inclusive indices into the pair's runs
 * as fg_align_ranges returns them; seq_divergence = float(range_err) / range_len, computed on the host.  An
 * OverlapRange piece is the parent record with the four coordinates and seq_divergence replaced (:416-417).
 * Arguments, ids and errors as fg_align_ranges; empty ranges give no records, n_pairs = 0 an empty batch.  Sub-batches
 * of pairs whose interval lists fit FG_TRIM_SCRATCH_BYTES (environment, default 1 GiB) are worked on at a time; a pair
 * beyond it runs alone, FG_ERR_NOMEM when the device cannot hold it (or a pair has more than 131072 runs). */
struct fg_trim_rec {
	int32_t cur_begin, cur_end, ext_begin, ext_end;
	int32_t run_start, run_end;
	int32_t range_err, range_len;
	float   seq_divergence;
};
struct fg_trim_batch { uint32_t n_pairs; uint64_t* rec_off; struct fg_trim_rec* recs; void* owner_; };
int fg_trim_ranges(fg_ctx* ctx, const struct fg_range_pair* pairs, uint32_t n_pairs, uint8_t use_hpc,
                   float max_divergence, int32_t min_overlap, struct fg_trim_batch* out);
void fg_release_trims(struct fg_trim_batch* b);

/* getAlignmentErrEdlib (src/sequence/alignment.cpp:218-247) for ranges of the resident sequences: what
 * ReadAligner::getChainBaseDivergence (src/repeat_graph/read_aligner.cpp:410-434) computes for every alignment of a
 * chain when reads_base_alignment is set.  Pairs, ids, containers and errors are those of fg_align_ranges: cur_id names
 * a sequence of the fg_set_queries container when one is set (the reads), otherwise of the indexed container; ext_id
 * always one of the indexed container (the graph edges); odd ids are the reverse-complement strand; empty ranges are
 * legal.  dist[i] = what edlibAlign(NW, TASK_DISTANCE, k = -1) returns for the two strings (alignment.cpp:233-238),
 * homopolymer-compressed first (alignment.cpp:52-70) when use_hpc != 0; an empty side gives the other side's length
 * (edlib.cpp:160-164).  len_cur / len_ext = the compared (compressed) lengths; divergence[i] = (float)dist /
 * (float)max(len_cur, len_ext), computed on the host from the integers (alignment.cpp:244), NaN for two empty
 * strings as the reference's expression gives.  dist is required with n_pairs > 0, the other three may be NULL;
 * n_pairs = 0 is FG_OK.  The strings are cut out of the 2-bit reads on the device by the kernels behind
 * nucl_alignment; only the side table (32 B per pair) goes up and 12 B per pair come back.  Pairs are worked on in
 * sub-batches of FG_EDIT_BATCH_PAIRS (environment, default 2^20); fg_kernel_times afterwards reports the sums over
 * them.  FG_ERR_STATE without reads; FG_ERR_ARG for an unknown id, begin < 0, end < begin, end > length, or NULL
 * pairs / dist with n_pairs > 0 -- found before any device work.  The context is left as fg_overlaps expects it. */
int fg_edit_ranges(fg_ctx* ctx, const struct fg_range_pair* pairs, uint32_t n_pairs, uint8_t use_hpc,
                   int32_t* dist, int32_t* len_cur, int32_t* len_ext, float* divergence);

/* ReadAligner::getChainBaseDivergence (read_aligner.cpp:410-434) from per-alignment values; host only, no context.
 * Chain c = the entries [chain_off[c], chain_off[c + 1]) of cur_range (the alignment's curRange()) and divergence
 * (the record's own seq_divergence for a caller that does not realign, fg_edit_ranges' divergence for one that does).
 * The reference's float sequence, every operation rounded to single precision on its own (no fused multiply-add):
 * sum = 0.0f, len = 0; per entry sum = sum + (float)cur_range[i] * (1.0f - divergence[i]), len += cur_range[i];
 * out[c] = 1.0f - sum / (float)len -- NaN for an empty chain or one of total length 0, as in the reference.
 * FG_ERR_ARG for NULL arrays with n_chains > 0 or decreasing offsets. */
int fg_chain_divergence(const int32_t* cur_range, const float* divergence, const uint64_t* chain_off,
                        uint32_t n_chains, float* out);

/* The edge-chain step of ReadAligner::alignReads (read_aligner.cpp:212-262) for a batch of reads: the lambda's filter
 * (:224-226), its std::sort by curBegin (:233-235) and chainReadAlignments (:24-154) -- the DP over the read's
 * alignments with its two deques and their cleanup, the std::sort of "active then frozen" by score (:119-123) and the
 * greedy selection of non-intersecting chains (:126-151).  What comes back is what chainReadAlignments returns, before
 * the divergence gate of :238-249 (fg_edit_ranges / fg_chain_divergence give the caller that).
 * recs[query_off[q] .. query_off[q + 1]) are the overlap records of query q in any order (fg_overlaps with only_max_ext
 * = 0, a scheduler result, a loaded dump); node_left[i] / node_right[i] are the caller's numbers of edge->nodeLeft /
 * nodeRight of the edge that owns indexed sequence first_ext_id + i, both strands listed (an odd id carries the
 * complement edge's nodes, idToSegment of :165-175).  Per query: a record is kept when ext_len < long_edge ||
 * min(cur_end - cur_begin, ext_end - ext_begin) > big_alignment; the kept ones are sorted by cur_begin and the chains
 * by score in the permutations libstdc++'s std::sort produces, ties included; scores add in int32.  Chains of query q:
 * chain_off[q] .. chain_off[q + 1], in the order chainReadAlignments returns them; alignments of chain c: aln[aln_off[c]
 * .. aln_off[c + 1]), indices into recs, front of the chain first; score[c] = Chain::score.
 * The step reads seven integers per record; only that table and the node tables go up and only the chains come back.
 * The context lends its device and stream: no reads, no index are needed, and any member of a group serves.  Queries
 * are worked on in sub-batches of FG_READCHAIN_BATCH_RECS records (environment, default 2^20; a longer query runs
 * alone); fg_kernel_times afterwards reports the sums over them.  A query may have at most FG_CHAIN_MAX_RECS records:
 * the DP is serial over a query's alignments.
 * FG_ERR_ARG, found before any device work: NULL p or out; NULL recs, query_off or node tables with records to read; a
 * decreasing query_off; max_jump <= 0 or another parameter < 0; a query beyond FG_CHAIN_MAX_RECS; a record whose ext_id
 * is outside [first_ext_id, first_ext_id + n_ext_ids) or with cur_begin < 0, cur_end < cur_begin, ext_begin < 0,
 * ext_end < ext_begin or ext_end > ext_len.  n_queries = 0 gives an empty batch (chain_off = {0}, aln_off = {0}). */
#define FG_CHAIN_MAX_RECS 65536
struct fg_chain_params {
	int32_t max_jump;          /* Config "maximum_jump"            (read_aligner.cpp:27) */
	int32_t max_read_overlap;  /* MAX_READ_OVLP = 50               (:28) */
	int32_t min_alignment;     /* Parameters::minimumOverlap       (:29) */
	int32_t max_separation;    /* Config "max_separation"          (:30) */
	int32_t long_edge;         /* LONG_EDGE = 900                  (:160) */
	int32_t big_alignment;     /* BIG_ALN = 500                    (:159) */
};
struct fg_chain_batch {
	uint32_t  n_queries;
	uint64_t  n_chains, n_alns;
	uint64_t* chain_off;   /* n_queries + 1: chains of query q, in the order chainReadAlignments returns them */
	uint64_t* aln_off;     /* n_chains + 1, into aln */
	uint64_t* aln;         /* index into the caller's recs[], front of the chain first */
	int32_t*  score;       /* n_chains: Chain::score */
	void*     owner_;
};
int fg_chain_alignments(fg_ctx* ctx, const struct fg_chain_params* p,
                        const struct fg_overlap_rec* recs, const uint64_t* query_off, uint32_t n_queries,
                        uint32_t first_ext_id, uint32_t n_ext_ids,
                        const uint32_t* node_left, const uint32_t* node_right,
                        struct fg_chain_batch* out);
void fg_release_chains(struct fg_chain_batch* b);

/* Window coverage of a read by its overlaps, and what ChimeraDetector reads off it (src/assemble/chimera.cpp:31-343).
 * One pass serves getReadCoverage (:106-134) and getCachedCoverage (:280-343): recs[query_off[q] .. query_off[q + 1])
 * are the overlap records of query q, in any order.  A record with ext_id == cur_id or ext_id == (cur_id ^ 1) is
 * skipped (:120-121).  Every other one adds 1 to the windows cur_begin / window .. cur_end / window - 2 inclusive
 * (:125-130 with FLANK = 1; nothing when the upper bound is below the lower) of `full` when lrOverhang() =
 * max(min(cur_begin, ext_begin), min(cur_len - cur_end, ext_len - ext_end)) (overlap.h:195-199) <= max_overhang, of
 * `junction` otherwise.  `full` over lazySeqOverlaps records is getReadCoverage's vector -- IterNoOverhang
 * (overlap.h:456-523) drops exactly the records that land in `junction`; `full` and `junction` over
 * quickSeqOverlaps(id, 0, force_local = true) records are getCachedCoverage's two vectors (:302-322).
 * Windows of a query: fg_coverage_windows below (the reference's float expression; a query of n <= 0 windows has one
 * window holding 0 and degenerate = 1).  sum / max / median / min_good are taken of `full` (:145-152, :166-182);
 * threshold and chimeric are fg_coverage_verdict's, computed on the host from those integers: no float runs on the
 * device.  Windows past the vector's end (the reference's .at() would throw; reachable only where (float)cur_len
 * rounds down, above 2^24 bp) are not counted.
 * The context lends its device and stream: no reads and no index are needed.  Queries are worked on in sub-batches of
 * FG_COVERAGE_BATCH_RECS records (environment, default 2^20; a longer query runs alone); fg_kernel_times afterwards
 * reports the sums over them.  FG_COVERAGE_TILE (windows per LDS tile, 64 .. 2048) and FG_COVERAGE_WAVE_MAX (the largest
 * window count a single wave takes, 0 .. 512; 0: every query takes a workgroup) are switches for tests.
 * FG_ERR_ARG, found before any device work: NULL p or out; NULL recs, query_off or query_len with something to read; a
 * decreasing query_off; window <= 0, max_overhang < 0, !(max_drop_rate > 0) or query_len[q] < 0; a record with
 * cur_len != query_len[q], cur_begin < 0, cur_end < cur_begin, cur_end > cur_len, ext_begin < 0, ext_end < ext_begin
 * or ext_end > ext_len.  n_queries = 0 gives an empty batch (win_off = {0}). */
struct fg_coverage_params {
	int32_t window;            /* Config "chimera_window"            (chimera.cpp:110, :294) */
	int32_t max_overhang;      /* Config "maximum_overhang"          (overlap.h:467, chimera.cpp:168, :295) */
	float   max_drop_rate;     /* Config "max_coverage_drop_rate"    (chimera.cpp:140) */
	int32_t overlap_coverage;  /* ChimeraDetector::_overlapCoverage; read when uneven_coverage == 0 */
	uint8_t uneven_coverage;   /* Parameters::get().unevenCoverage   (chimera.cpp:156) */
	uint8_t want_vectors;      /* 0: only the per-read values come back */
	uint8_t pad_[2];
};
struct fg_coverage_batch {
	uint32_t  n_queries;
	uint64_t* win_off;     /* n_queries + 1: windows of query q = win_off[q+1] - win_off[q] (always >= 1) */
	int32_t*  full;        /* want_vectors: records with lrOverhang() <= max_overhang */
	int32_t*  junction;    /* want_vectors: records with lrOverhang() >  max_overhang */
	int64_t*  sum;         /* of full   (sumCov, chimera.cpp:146-151) */
	int32_t*  max;         /* of full   (maxCov) */
	int32_t*  median;      /* of full   (utils.h:32-51: sorted[min(n * 50 / 100, n - 1)]) */
	int32_t*  min_good;    /* min of full[max_flank .. n - max_flank - 1]; INT32_MAX when that range is empty */
	int32_t*  threshold;   /* chimera.cpp:155-164 */
	uint8_t*  chimeric;    /* testReadByCoverage's return value */
	uint8_t*  degenerate;  /* 1: numWindows - 2 <= 0 -- getReadCoverage returns {0}, getCachedCoverage throws */
	void*     owner_;
};
int  fg_read_coverage(fg_ctx* ctx, const struct fg_coverage_params* p, const struct fg_overlap_rec* recs,
                      const uint64_t* query_off, uint32_t n_queries, const int32_t* query_len,
                      struct fg_coverage_batch* out);
void fg_release_coverage(struct fg_coverage_batch* b);

/* The two float steps of the above; host only, no context.
 * fg_coverage_windows: numWindows = std::ceil((float)seq_len / window) + 1 in single precision, converted to int
 * (chimera.cpp:114, :298 -- (float)seq_len rounds above 2^24 bp; this is the only place the expression is written);
 * n = numWindows - 2; *n_windows = n, or 1 with *degenerate = 1 when n <= 0 (:115); *max_flank =
 * (int)((float)max_overhang / (float)window) (:168-169).  Any of the three pointers may be NULL.  FG_ERR_ARG for
 * seq_len < 0, window <= 0 or max_overhang < 0.
 * fg_coverage_verdict: testReadByCoverage's decision (:153-182) for n vectors from their integers: chimeric = 1 and
 * threshold = 0 when sum == 0; otherwise threshold = (int)std::max(1L, std::lround(x / max_drop_rate)) with x =
 * (float)overlap_coverage, or the median converted to float when uneven_coverage is set; good_start = max_flank,
 * good_end = n_windows - max_flank - 1, chimeric = good_end <= good_start || min_good < threshold.  threshold may be
 * NULL.  FG_ERR_ARG for NULL p, a NULL array with n > 0, window <= 0, max_overhang < 0 or !(max_drop_rate > 0). */
int fg_coverage_windows(int32_t seq_len, int32_t window, int32_t max_overhang, int32_t* n_windows, int32_t* max_flank,
                        uint8_t* degenerate);
int fg_coverage_verdict(const struct fg_coverage_params* p, uint32_t n, const int32_t* n_windows, const int64_t* sum,
                        const int32_t* median, const int32_t* min_good, int32_t* threshold, uint8_t* chimeric);

/* Window coverage of the graph edges by the read paths: the first half of MultiplicityInferer::estimateCoverage
 * (src/repeat_graph/multiplicity_inferer.cpp:14-41) and the median of :63.  Path p is aln[aln_off[p] .. aln_off[p + 1]),
 * indices into recs (n_recs of them), front of the path first: the layout of fg_chain_batch.  edge_of[i] is the
 * caller's edge number of indexed sequence first_ext_id + i, edge_len[e] its GraphEdge::length()
 * (repeat_graph.h:118-128); edge e has size = edge_len[e] / window windows (integer division; may be 0).  Position j
 * of a path of m alignments adds 1 to the windows [from, to) of its edge, from = (j > 0) ? 0 : max(0, ext_begin /
 * window + 1), to = (j < m - 1) ? size : min(size, ext_end / window) (:32-39); nothing when from >= to.  Per edge: the
 * vector (want_vectors), its sum, max and median (0 for an empty vector, utils.h:34).  _meanCoverage, the
 * complement-edge average and the quantile of :43-88 are a few integer operations over these and stay with the
 * caller.  One call is one device batch (at most 2^30 - 1 path elements); the context lends its device and stream.
 * FG_ERR_ARG, found before any device work: NULL out; window <= 0; an aln index >= n_recs; an ext_id outside
 * [first_ext_id, first_ext_id + n_ext_ids); edge_of[i] >= n_edges; edge_len[e] < 0; a decreasing aln_off; a NULL
 * array where something must be read.  n_edges = 0 gives an empty batch (win_off = {0}). */
struct fg_edge_coverage_batch {
	uint32_t  n_edges;
	uint64_t* win_off;     /* n_edges + 1: edge_len[e] / window windows (integer division; may be 0) */
	int32_t*  cov;         /* want_vectors */
	int64_t*  sum; int32_t* max; int32_t* median;   /* median of an empty vector is 0 (utils.h:34) */
	void*     owner_;
};
int  fg_edge_coverage(fg_ctx* ctx, int32_t window, const struct fg_overlap_rec* recs, uint64_t n_recs,
                      const uint64_t* aln, const uint64_t* aln_off, uint64_t n_paths,
                      uint32_t first_ext_id, uint32_t n_ext_ids, const uint32_t* edge_of,
                      uint32_t n_edges, const int32_t* edge_len, uint8_t want_vectors,
                      struct fg_edge_coverage_batch* out);
void fg_release_edge_coverage(struct fg_edge_coverage_batch* b);

/* Bubble polishing: what flye-modules polisher does to every bubble (src/polishing: BubbleProcessor::parallelWorker,
 * GeneralPolisher::polishBubble / makeStep, Alignment, DinucleotideFixer::fixBubble; HomoPolisher is switched off in the
 * reference, bubble_processor.cpp:99, and is not here).
 * Bytes fall into six classes: 'A' 0, 'C' 1, 'G' 2, 'T' 3, '-' 5 (gap), every other byte below 128 class 4 (lower case
 * too: the reference's file reader upper-cases, this call does not).  score[c][r] is the score of consensus class c
 * against read class r: score[x][x] = mat x, score[x][y] = mis x->y, score[x][5] = del x, score[5][y] = ins y; the
 * reference leaves every other pair at 0, so row and column 4 and score[5][5] are 0 in a loaded matrix.
 * For a candidate v (length L) and a branch w (length Lb): F[i][j] = the best score of v[0:i] against w[0:j] (F[0][0] =
 * 0, borders by del / ins, inside max of left + ins, up + del, diagonal + score), R the same for the last i bases of v
 * against the last j of w.  A(v) = sum over the branches of F[L][Lb], where a branch counts 0 when L = 0 or Lb = 0
 * (alignment.cpp:150-190 returns its untouched local).  makeStep (general_polisher.cpp:60-123): the deletions of v[p]
 * (max_j F[p][j] + R[L-1-p][Lb-j]), p ascending, the first maximum above A(v) wins; only if none improves the
 * insertions of A, C, G, T before p = 0 .. L (sub[0] = F[p][0] + del b, sub[j+1] = max(F[p][j] + score[b][w[j]],
 * F[p][j+1] + del b); max_j sub[j] + R[L-p][Lb-j]); only if none improves the substitutions of v[p] by every letter
 * that differs from it (the same sub against R[L-1-p]).  optimize (:10-35) repeats makeStep and records every step;
 * it stops when a step changes nothing, when a step's score is > 0 (status bit 1) or when more than 10 * len(v0)
 * earlier iterations have run (bit 2); in the last two cases the step is recorded and the candidate from before it
 * stays.  A bubble of more than 10 branches is first optimized against five of them: std::sort by length (libstdc++'s
 * permutation), positions [n/2 - 2, n/2 + 3).  Then fixBubble (fix_dinucleotides != 0): the longest run (>= 3) of a pair
 * of two different bases that a different pair ends (shift 0 before shift 1, the first longest) is lengthened by one
 * pair if that raises A, else shortened by one pair if that raises A (bit 3, one more step of score 0).  A bubble with
 * a candidate of 5000 bytes or more, or with fewer than two branches, comes back unchanged without steps (bit 0).
 * Bubble i: candidate cand[cand_off[i] .. cand_off[i+1]), branches bubble_branch_off[i] .. bubble_branch_off[i+1],
 * branch r = branches[branch_off[r] .. branch_off[r+1]).
 * The context lends its device and stream: no reads and no index are needed.  The host drives the step loop; each
 * round works on the bubbles still at work in chunks of at most FG_POLISH_SCRATCH_BYTES of scratch (environment,
 * default 8 GiB; 16 bytes per cell of (L + 1) * (Lb + 1) per branch plus 72 (L + 1)); FG_POLISH_BATCH_BUBBLES (a switch
 * for tests) also bounds the bubbles of a chunk.  The result does not depend on either.  fg_kernel_times afterwards
 * reports the sums over all rounds.
 * FG_ERR_ARG, found before any device work: NULL matrix or out; a NULL array with n_bubbles > 0; an offset array that
 * decreases; a byte >= 128 in a candidate or a branch.  FG_ERR_NOMEM: one bubble alone needs more than the scratch
 * budget.  n_bubbles = 0 gives an empty batch (cand_off = {0}). */
struct fg_subs_matrix { int64_t score[6][6]; };
struct fg_polish_batch {
	uint32_t  n_bubbles;
	uint8_t*  cand;          /* the polished candidates, bubble i at cand_off[i] .. cand_off[i+1] */
	uint64_t* cand_off;      /* n_bubbles + 1 */
	uint32_t* n_steps;       /* recorded steps of bubble i (both optimize phases and the fixer) */
	uint8_t*  status;        /* bit 0 skipped, 1 stopped on score > 0, 2 stopped on the iteration limit, 3 fixer changed it */
	uint64_t* step_off;      /* want_steps: n_bubbles + 1, the steps of bubble i are step_off[i] .. step_off[i+1] */
	int64_t*  step_score;    /* want_steps */
	uint8_t*  step_seq;      /* want_steps: step t at step_seq_off[t] .. step_seq_off[t+1] */
	uint64_t* step_seq_off;  /* want_steps: number of steps + 1 */
	void*     owner_;
};
/* Host only, no context: reads the reference's *_substitutions.mat text (tab-separated "mat X p", "mis X->Y p",
 * "del X p", "ins X p"; other lines are ignored, a trailing \r is dropped); score = (int64)round(log(p) * 131072) in
 * double.  FG_ERR_ARG: NULL arguments, a file that cannot be read, a line of those four kinds that is malformed or
 * names a letter outside A, C, G, T. */
int  fg_subs_matrix_load(const char* path, struct fg_subs_matrix* out);
int  fg_polish_bubbles(fg_ctx* ctx, const struct fg_subs_matrix* matrix, const uint8_t* cand, const uint64_t* cand_off,
                       const uint8_t* branches, const uint64_t* branch_off, const uint64_t* bubble_branch_off,
                       uint32_t n_bubbles, uint8_t fix_dinucleotides, uint8_t want_steps, struct fg_polish_batch* out);
void fg_release_polish(struct fg_polish_batch* b);

/* The bubble partition of the reference's polisher: what _thread_worker (flye/polishing/bubbles.py:64-73) does to one
 * contig from _compute_profile onward, for a batch of contigs: _compute_profile with both shift_gaps passes
 * (alignment.py:68-92), _get_partition, _get_bubble_seqs and _postprocess_bubbles.  The output is, field for field, what
 * fg_polish_bubbles takes (the reference's polisher reads its bubbles file upper-cased; this call keeps case).
 * params are cfg.vals of flye/config/py_cfg.py:41-46 and the err_modes entry of the platform (:52-66).
 * Contig i has contig_len[i] positions, contig_circular[i] != 0 where contig_info.type == "circular" (NULL: none is), and
 * the alignments contig_aln_off[i] .. contig_aln_off[i+1], in the order of the reference's list (it decides nucl and the
 * order and cap of the branches).  Alignment a: trg_start, trg_end, err_rate (the parser's value, not recomputed) and
 * the gapped strings aln.trg_seq / aln.qry_seq as the columns col_off[a] .. col_off[a+1] of trg_cols / qry_cols, one byte
 * per column, '-' the gap.  Offsets need not start at zero.
 * shift_gaps: a gap run [a, b) of the second string moves left by m columns and the m bases before it move, in order, to
 * [b - m, b); m = the number of k < min(b - a, a) in a row with second[a-1-k] == first[b-1-k].  Runs are handled left to
 * right on the bytes earlier runs left; a run that reaches the end closes there (the "$" sentinels do that and stop the
 * walk at the first column).  Profile (:273-314): only alignments with !(err_rate > max_aln_error) && columns >=
 * min_polish_aln_len, shifted strings; a column with a target gap counts into num_inserts of the position before it
 * (before position 0: contig_len - 1); any other column sets nucl (the last alignment in list order wins), adds to
 * coverage, to num_deletions on a query gap, else to num_missmatch when the bytes differ; positions wrap at contig_len.
 * A position is good when coverage > 0, (num_missmatch + num_deletions) / coverage <= solid_missmatch and num_inserts /
 * coverage <= solid_indel in double (the host tabulates, per coverage, the largest numerator that passes).  Partition
 * (:317-359): in a maximal run of good positions [s, e] the first min(floor((e-s+1) / SOLID), floor((len-SOLID-1-s) /
 * SOLID) + 1) * SOLID positions are solid (none when s >= len - SOLID); prof_pos walks from SOLID while < len - SOLID,
 * appends prof_pos + SIMPLE / 2 and jumps by SOLID at a landmark (SIMPLE solid positions and _is_simple_kmer) or when
 * prof_pos - prev_partition > max_bubble_length (n_long_bubbles counts the latter).  Bubbles (:362-412): none without a
 * partition; ALL alignments, ORIGINAL strings; a cut is a non-gap target column at position 0 or at a partition point
 * (not the first non-gap column unless it is position 0); a cut gives the query bytes since the previous cut (since the
 * string's start for the first), without gaps and through to_acgt (fasta_parser.py:217-219), to the bubble that was
 * current, if a cut came before or the alignment starts in bubble 0 of a linear contig; trg_end > partition[-1] on a
 * linear contig appends the rest to the last bubble.  Post-processing (:175-217) in integers: median = element n / 2 of
 * the order (length, index); 2 * med > 3 * max_bubble_length keeps the median alone; else 2 * |len - med| < med stays;
 * |med - len(consensus)| > med / 2 replaces the consensus; at most max_bubble_branches stay.
 * The context lends its device and stream: no reads and no index are needed.  The call works in sub-batches of whole
 * contigs of at most FG_BUBBLE_BATCH_COLS (environment, default 2^27) columns plus positions and, as a switch for tests,
 * of at most FG_BUBBLE_BATCH_CONTIGS contigs; the result does not depend on either.  FG_ERR_NOMEM: a contig that alone exceeds it.  FG_ERR_UNSUPPORTED: simple_kmer_length odd, < 2, > 2 *
 * solid_kmer_length or 3 * simple_kmer_length / 2 > solid_kmer_length + 1 (the reference's slices would leave the
 * profile).  FG_ERR_ARG, found before any device work: NULL params or out; a NULL array where something must be read; an
 * offset array that decreases; a byte >= 128; contig_len < 0; trg_start outside [0, contig_len); an alignment with more
 * non-gap target columns than contig_len; a length or cap <= 0; a rate (err_rate too) that is NaN or negative.
 * n_contigs = 0 gives an empty batch. */
struct fg_bubble_params {
	int32_t solid_kmer_length, simple_kmer_length, max_bubble_length, max_bubble_branches, min_polish_aln_len, pad_;
	double  solid_missmatch, solid_indel, max_aln_error;
};
struct fg_bubble_batch {
	uint32_t  n_contigs;
	uint32_t  n_bubbles;
	uint64_t  n_alignments;
	uint64_t* bubble_off;         /* n_contigs + 1: the bubbles of contig i */
	int32_t*  position;           /* n_bubbles */
	uint8_t*  cand;               /* the consensus of bubble b at cand_off[b] .. cand_off[b+1] */
	uint64_t* cand_off;           /* n_bubbles + 1 */
	uint8_t*  branches;
	uint64_t* branch_off;         /* number of branches + 1 */
	uint64_t* bubble_branch_off;  /* n_bubbles + 1 */
	int32_t*  n_long_bubbles;     /* per contig */
	int32_t*  n_empty;
	int32_t*  n_long_branch;
	int64_t*  mean_cov;           /* sum(len(b.branches)) // (bubbles + 1) BEFORE post-processing (:71) */
	int32_t*  n_partition;
	uint8_t*  in_profile;         /* n_alignments: 1 where the alignment passed the filter of :283 */
	uint64_t* part_off;           /* want_profile: n_contigs + 1 */
	int32_t*  partition;          /* want_profile */
	uint64_t* prof_off;           /* want_profile: n_contigs + 1, into the five arrays below */
	int32_t*  coverage;
	int32_t*  num_inserts;
	int32_t*  num_deletions;
	int32_t*  num_missmatch;
	uint8_t*  nucl;               /* 0: no base */
	void*     owner_;
};
int  fg_make_bubbles(fg_ctx* ctx, const struct fg_bubble_params* params, uint32_t n_contigs, const int32_t* contig_len,
                     const uint8_t* contig_circular, const uint64_t* contig_aln_off, const int32_t* trg_start,
                     const int32_t* trg_end, const double* err_rate, const uint64_t* col_off, const uint8_t* trg_cols,
                     const uint8_t* qry_cols, uint8_t want_profile, struct fg_bubble_batch* out);
void fg_release_bubbles(struct fg_bubble_batch* b);

/* get_uniform_alignments (flye/polishing/alignment.py:95-153): the per-window coverage cap that both _contig_profile
 * (consensus.py:114) and make_bubbles call first, for a batch of contigs in the layout of fg_make_bubbles.  Contig i has
 * n_w = contig_len[i] / 100 + 1 windows and the alignments contig_aln_off[i] .. contig_aln_off[i+1]; alignment a covers the
 * windows [trg_start / 100, trg_end / 100) (none when trg_end < trg_start, as on a circular contig), adds its err_rate to
 * the list of each and, unless is_secondary[a] (NULL: none is), one to wnd_primary_cov.  With s the sorted primary
 * coverages and m2 twice their median (2 s[n_w / 2] for odd n_w, else s[n_w / 2 - 1] + s[n_w / 2]), cov_threshold =
 * max(5 * m2 / 8, 10) in integers: the reference's int(1.25 * median) is exact in double for these values.  A window of
 * more than cov_threshold entries has the threshold element cov_threshold of its ascending list, else 1.0; keep[a] = 1
 * when good > floor(total / 2), good = the alignment's windows with err_rate <= threshold, total = trg_end / 100 -
 * trg_start / 100 (an alignment inside one window is dropped, one with negative total is kept).  All compares are exact.
 * want_thresholds also returns the windows' thresholds, contig i at wnd_off[i] .. wnd_off[i+1].
 * The context lends its device and stream.  Sub-batches of whole contigs of at most FG_UNIFORM_BATCH_PAIRS (environment,
 * default 2^26) (alignment, window) pairs; the result does not depend on the cut; FG_ERR_NOMEM: a contig that alone needs
 * more.  FG_ERR_ARG, found before any device work: NULL where something is read; decreasing offsets; contig_len < 0;
 * trg_start < 0 or trg_end < 0; max(trg_start, trg_end) / 100 > contig_len / 100 (the reference raises IndexError); an
 * err_rate that is NaN or negative.  n_contigs = 0 gives an empty result. */
struct fg_uniform_result {
	uint32_t  n_contigs;
	uint32_t  pad_;
	uint64_t  n_alignments;
	uint8_t*  keep;               /* n_alignments, from contig_aln_off[0] on */
	int32_t*  cov_threshold;      /* per contig */
	uint64_t* wnd_off;            /* want_thresholds: n_contigs + 1 */
	double*   wnd_threshold;      /* want_thresholds */
	void*     owner_;
};
int  fg_uniform_alignments(fg_ctx* ctx, uint32_t n_contigs, const int32_t* contig_len, const uint64_t* contig_aln_off,
                           const int32_t* trg_start, const int32_t* trg_end, const double* err_rate,
                           const uint8_t* is_secondary, uint8_t want_thresholds, struct fg_uniform_result* out);
void fg_release_uniform(struct fg_uniform_result* r);

/* The reference's consensus stage (flye/polishing/consensus.py:108-181: _contig_profile after get_uniform_alignments, and
 * _flatten_profile) for a batch of contigs.  The contig and alignment arrays are those of fg_make_bubbles (offsets need
 * not start at zero; trg_end and circularity are not read).  qry_id[a] is the caller's number for aln.qry_id: alignments
 * of one contig with the same number are the same read.  Only alignments with use[a] != 0 take part (NULL: all), in list
 * order: the keep[] of fg_uniform_alignments goes here as it is.
 * Both shift_gaps passes run first (see fg_make_bubbles).  A non-gap target column c lands at trg_start + c, wrapped once
 * at contig_len; a target-gap column at the position before it (before position 0: contig_len - 1).  A column with a
 * target gap and a query base appends the base to insertions[qry_id] of its position, in list order of the alignments,
 * then column order; every other column sets nucl to the target byte (the last writer wins; a gap against a gap sets '-')
 * and counts matches[query byte].  Per position: max_match = the smallest byte among those of the largest count (nucl
 * when nothing matched), max_insert = the most frequent insertion string, ties to the smallest in byte order (a proper
 * prefix is smaller); the sequence takes max_match unless it is '-', then max_insert when num_ins > match_total / 2
 * (num_ins = the reads with an insertion there, match_total = the sum of matches).  Bytes below 128, case kept.
 * want_profile also returns, per position, nucl ('-' where nothing set it), match_total, num_ins, max_match, accepted
 * (max_insert went into the sequence) and max_insert itself (empty without insertions) behind ins_off.
 * Sub-batches of whole contigs of at most FG_CONSENSUS_BATCH_COLS (environment, default 2^27) columns plus positions and,
 * as a switch for tests, FG_CONSENSUS_BATCH_CONTIGS contigs; the result depends on neither.  FG_ERR_NOMEM: a contig that
 * alone exceeds the budget.  FG_ERR_ARG, found before any device work: NULL out or a NULL array where something must be
 * read; an offset array that decreases; a byte >= 128; contig_len < 0; and, for an alignment in use (the positions of
 * the others are not looked at): trg_start outside [0, contig_len), more non-gap target columns than contig_len, a contig
 * of length 0.  n_contigs = 0 gives an empty batch (seq_off = {0}). */
struct fg_consensus_batch {
	uint32_t  n_contigs;
	uint32_t  pad_;
	uint64_t* seq_off;            /* n_contigs + 1 */
	uint8_t*  seq;                /* contig i at seq_off[i] .. seq_off[i+1], possibly empty */
	uint64_t* prof_off;           /* want_profile: n_contigs + 1, into the arrays below */
	uint8_t*  nucl;
	int32_t*  match_total;
	int32_t*  num_ins;
	uint8_t*  max_match;
	uint8_t*  accepted;
	uint64_t* ins_off;            /* positions + 1 */
	uint8_t*  ins;                /* max_insert of position p at ins_off[p] .. ins_off[p+1] */
	void*     owner_;
};
int  fg_contig_consensus(fg_ctx* ctx, uint32_t n_contigs, const int32_t* contig_len, const uint64_t* contig_aln_off,
                         const int32_t* trg_start, const int32_t* qry_id, const uint8_t* use, const uint64_t* col_off,
                         const uint8_t* trg_cols, const uint8_t* qry_cols, uint8_t want_profile,
                         struct fg_consensus_batch* out);
void fg_release_consensus(struct fg_consensus_batch* b);

/* SynchronizedSamReader._parse_cigar (flye/utils/sam_parser.py:260-323) for a batch of SAM records: the step that makes
 * the input of the three calls above.  Contig i is the bytes contig_off[i] .. contig_off[i+1] of contig_seq; alignment a
 * lies on contig aln_contig[a] at SAM POS ctg_pos[a] (1-based), has the CIGAR runs run_off[a] .. run_off[a+1] (run_op the
 * operation as its ASCII byte, run_len its length) and the SAM SEQ bytes read_off[a] .. read_off[a+1] of read_seq.
 * Offsets need not start at zero.  Per run, in order (:275-306): M appends the next run_len read bytes to qry_seq and the
 * next run_len contig bytes to trg_seq; I the read bytes against '-'; D '-' against the contig bytes; S advances the read
 * position and counts as left soft clip only while no operation other than H has come before, else as right soft clip,
 * wherever it stands; H counts as left hard clip only as the very first operation, else as right hard clip.  A run of
 * length 0 is legal and gives nothing.  Bytes are upper-cased as bytes.upper() does it (a-z only) and compared after that.
 * trg_start = ctg_pos - 1, trg_end = trg_start + the contig bytes consumed; with qry_pos the read bytes consumed (:316-320)
 * qry_start = left hard + left soft, qry_end = qry_pos + left hard - right soft, qry_len = qry_pos + left hard + right
 * hard.  matches = the columns with equal bytes (:310-313, counted on the device); err_rate = 1.0 - (double)matches /
 * (double)columns on the host, bit-equal to Python's 1 - matches / len.  The columns of alignment a are col_off[a] ..
 * col_off[a+1] of trg_cols / qry_cols, the layout fg_make_bubbles and fg_contig_consensus read; want_cols = 0 leaves both
 * NULL and still counts (for a caller that runs fg_uniform_alignments first and expands only what it keeps).
 * The context lends its device and stream: no reads and no index are needed.  The contig bytes go up once per call; the
 * call works in sub-batches of whole alignments of at most FG_CIGAR_BATCH_COLS columns (environment, default 2^27) and,
 * as a switch for tests, FG_CIGAR_BATCH_ALNS alignments; FG_CIGAR_TILE (columns per workgroup of k_cig_expand, a power of
 * two in 64 .. 4096, default 2048) is a switch for tests too.  The result depends on none of them.  FG_ERR_NOMEM: an
 * alignment that alone exceeds the column budget.  FG_ERR_UNSUPPORTED: an operation among N P = X (the reference raises
 * AlignmentException, :303).  FG_ERR_ARG, found before any device work: NULL out or a NULL array where something must be
 * read; an offset array that decreases; aln_contig >= n_contigs; ctg_pos < 1; any other operation byte; a byte >= 128 in
 * a contig or a read; an alignment whose runs consume more read bytes than its SEQ holds or walk past the end of its
 * contig (the reference silently returns strings of unequal length there; this call refuses); an alignment of zero
 * columns (the reference divides by zero, :314); totals that do not fit int32.  After an error *out is all zero.
 * n_alignments = 0 gives an empty batch (col_off = {0}). */
struct fg_expand_batch {
	uint64_t  n_alignments;
	uint64_t* col_off;            /* n_alignments + 1, starts at 0 */
	uint8_t*  trg_cols;           /* want_cols: aln.trg_seq, one byte per column, '-' the gap */
	uint8_t*  qry_cols;           /* want_cols: aln.qry_seq */
	int32_t  *trg_start, *trg_end, *qry_start, *qry_end, *qry_len;
	int64_t*  matches;            /* columns with equal bytes */
	double*   err_rate;           /* 1.0 - (double)matches / (double)columns, computed on the host */
	void*     owner_;
};
int  fg_expand_cigars(fg_ctx* ctx, uint32_t n_contigs, const uint64_t* contig_off, const uint8_t* contig_seq,
                      uint64_t n_alignments, const uint32_t* aln_contig, const int32_t* ctg_pos /* SAM POS, 1-based */,
                      const uint64_t* run_off, const uint8_t* run_op /* ASCII */, const uint32_t* run_len,
                      const uint64_t* read_off, const uint8_t* read_seq, uint8_t want_cols, struct fg_expand_batch* out);
void fg_release_expand(struct fg_expand_batch* b);

/* fg_expand_cigars(want_cols = 1) followed by fg_contig_consensus as ONE call: the columns are expanded on the device
 * straight into the buffers the consensus kernels read and never cross the bus.  The contig bytes are those of
 * fg_expand_cigars (contig_len[i] = contig_off[i+1] - contig_off[i]); the alignments are grouped by contig in the caller's
 * order as for fg_contig_consensus: contig i has the alignments contig_aln_off[i] .. contig_aln_off[i+1], which replaces
 * aln_contig.  ctg_pos, run_off, run_op, run_len, read_off and read_seq describe alignment a as for fg_expand_cigars,
 * qry_id, use and want_profile are those of fg_contig_consensus; every per-alignment array is indexed by the caller's
 * alignment number, and no offset array need start at zero.  Every field of *out equals what the two calls give for the
 * same records; it is released with fg_release_consensus.
 * Sub-batches of whole contigs under the budgets of fg_contig_consensus (FG_CONSENSUS_BATCH_COLS columns plus positions,
 * FG_CONSENSUS_BATCH_CONTIGS); a sub-batch also ends where the expansion's numbering does (2^31 - 1 columns, runs and SEQ
 * bytes, 2^30 - 1 alignments).  Each sub-batch expands its own alignments (FG_CIGAR_TILE applies, FG_CIGAR_BATCH_COLS
 * and FG_CIGAR_BATCH_ALNS do not); the contig bytes go up once per call.  The set of query bytes that sizes the match
 * table is found on the device (k_col_present), over the alignments in use only, as the host finds it in the two-step
 * path.  The result depends on none of the switches.
 * Errors: every code of fg_expand_cigars for the same records (FG_ERR_UNSUPPORTED for N P = X; FG_ERR_ARG for NULL where
 * something is read, decreasing offsets, ctg_pos < 1, runs that overrun SEQ or the contig, an alignment without columns,
 * a byte >= 128, totals beyond int32), then those of fg_contig_consensus that the expansion does not already exclude
 * (FG_ERR_ARG: an alignment in use whose trg_start is not inside its contig, which only an alignment of insertions alone
 * behind the last base can be; a contig of 2^31 bytes), all found before any device work.  FG_ERR_NOMEM: a contig that
 * alone exceeds FG_CONSENSUS_BATCH_COLS or the expansion's numbering (the message names the switch), a match table of
 * 2^32 cells.  After an error *out is all zero and the context stays usable.  n_contigs = 0 gives an empty batch. */
int  fg_contig_consensus_cigars(fg_ctx* ctx, uint32_t n_contigs, const uint64_t* contig_off, const uint8_t* contig_seq,
                                const uint64_t* contig_aln_off, const int32_t* ctg_pos /* SAM POS, 1-based */,
                                const uint64_t* run_off, const uint8_t* run_op /* ASCII */, const uint32_t* run_len,
                                const uint64_t* read_off, const uint8_t* read_seq, const int32_t* qry_id, const uint8_t* use,
                                uint8_t want_profile, struct fg_consensus_batch* out);

/* fg_expand_cigars(want_cols = 1) followed by fg_make_bubbles as ONE call, with the same substitutions as
 * fg_contig_consensus_cigars: contig bytes for contig_len, contig_aln_off for aln_contig, the records for the columns;
 * trg_start = ctg_pos - 1 and trg_end = trg_start + the contig bytes the runs consume.  params, contig_circular and
 * want_profile are those of fg_make_bubbles.  err_rate stays an input (the caller has it from the want_cols = 0 expansion
 * it made for fg_uniform_alignments): it decides in_profile before any column exists.  Every field of *out equals what the
 * two calls give for the same records and the same err_rate; it is released with fg_release_bubbles.
 * Sub-batches of whole contigs under FG_BUBBLE_BATCH_COLS / FG_BUBBLE_BATCH_CONTIGS and the expansion's numbering, as
 * above.  Errors: those of fg_make_bubbles for the parameters and err_rate, every code of fg_expand_cigars for the
 * records, FG_ERR_ARG for an alignment whose trg_start is not inside its contig and for a contig of 2^31 bytes;
 * FG_ERR_NOMEM as above with FG_BUBBLE_BATCH_COLS.  After an error *out is all zero and the context stays usable.
 * n_contigs = 0 gives an empty batch. */
int  fg_make_bubbles_cigars(fg_ctx* ctx, const struct fg_bubble_params* params, uint32_t n_contigs, const uint64_t* contig_off,
                            const uint8_t* contig_seq, const uint8_t* contig_circular, const uint64_t* contig_aln_off,
                            const int32_t* ctg_pos /* SAM POS, 1-based */, const uint64_t* run_off,
                            const uint8_t* run_op /* ASCII */, const uint32_t* run_len, const uint64_t* read_off,
                            const uint8_t* read_seq, const double* err_rate, uint8_t want_profile, struct fg_bubble_batch* out);

/* host only, no context: the tokens of the reference's re "[0-9]+[MIDNSHP=X]" (:140) in order, as findall gives them
 * (bytes that match nothing are skipped).  *n_runs = the number of tokens; at most cap of them are written.  FG_ERR_ARG:
 * more tokens than cap (*n_runs still says how many), a length beyond uint32, NULL n_runs, NULL where something is read
 * or written. */
int  fg_cigar_parse(const char* cigar, uint64_t n_bytes, uint8_t* ops, uint32_t* lens, uint64_t cap, uint64_t* n_runs);

/* Trestle's divergent positions (flye/trestle/divergence.py:55-143: _contig_profile, _count_freqs and _call_position) for a
 * batch of contigs.  The contig and alignment arrays are those of fg_make_bubbles and fg_contig_consensus (offsets need
 * not start at zero).  Every alignment takes part, in list order: there is no uniform step and no error filter.
 * Both shift_gaps passes run first (see fg_make_bubbles).  A non-gap target column c lands at trg_start + c, wrapped once
 * at contig_len; a target-gap column at the position before it, and before position 0 that is contig_len - 1: Python's
 * index -1 is the last element.  A target-gap column counts insertions[query byte] of its position for that one byte (a
 * '-' against a '-' counts insertions['-']); every other column sets nucl to the target byte (the last alignment in list
 * order wins) and counts matches[query byte].  Per position: cov = the sum of matches; mat_ct = matches[nucl]; del_ct =
 * matches['-']; (sub_base, sub_ct) = the key of the largest count among the keys of matches other than nucl and '-';
 * (ins_base, ins_ct) likewise among all keys of insertions ('-' included).  Ties of the largest count go to the key that
 * entered the reference's dict first, as max(d, key=d.get) returns it: the alignment earliest in list order, then the
 * earliest column -- not the smallest byte.  Without a key sub_base / ins_base are 0 and the count is 0.
 * A position with cov != 0 is called for substitutions when sub_ct / (double)cov >= sub_thresh in double, and likewise
 * for deletions (del_ct) and insertions (ins_ct, which may exceed cov): flags = 1 (sub) | 2 (del) | 4 (ins).  The device
 * does not divide: it compares with the smallest passing count per coverage, tabulated on the host.  The four lists hold
 * the positions (indices inside the contig, ascending) with any flag, flag 1, flag 2 and flag 4; contig i's part of a
 * list lies at x_off[i] .. x_off[i+1].  want_profile also returns the values above per position behind prof_off (nucl is
 * '-' where nothing set it).  Bytes below 128, case kept.
 * The context lends its device and stream: no reads and no index are needed.  Sub-batches of whole contigs of at most
 * FG_DIVERGENCE_BATCH_COLS (environment, default 2^27) columns plus positions times the number of distinct query bytes of
 * the call and, as a switch for tests, FG_DIVERGENCE_BATCH_CONTIGS contigs; the result depends on neither.  FG_ERR_NOMEM:
 * a contig that alone exceeds the budget.  FG_ERR_ARG, found before any device work: NULL out or a NULL array where
 * something must be read; an offset array that decreases; a byte >= 128; contig_len < 0; trg_start outside
 * [0, contig_len); more non-gap target columns than contig_len; a threshold that is NaN or negative.  After an error *out
 * is all zero.  n_contigs = 0 gives an empty batch (every offset array = {0}). */
struct fg_divergence_batch {
	uint32_t  n_contigs;
	uint32_t  pad_;
	uint64_t* total_off;          /* n_contigs + 1, likewise sub_off, del_off, ins_off */
	int32_t*  total_pos;          /* positions with any flag */
	uint64_t* sub_off;
	int32_t*  sub_pos;
	uint64_t* del_off;
	int32_t*  del_pos;
	uint64_t* ins_off;
	int32_t*  ins_pos;
	uint64_t* prof_off;           /* want_profile: n_contigs + 1, into the arrays below */
	int32_t*  cov;
	uint8_t*  nucl;
	int32_t*  mat_ct;
	uint8_t*  sub_base;           /* 0: none */
	int32_t*  sub_ct;
	int32_t*  del_ct;
	uint8_t*  ins_base;           /* 0: none */
	int32_t*  ins_ct;
	uint8_t*  flags;              /* 1 sub | 2 del | 4 ins */
	void*     owner_;
};
int  fg_divergence_profile(fg_ctx* ctx, double sub_thresh, double del_thresh, double ins_thresh, uint32_t n_contigs,
                           const int32_t* contig_len, const uint64_t* contig_aln_off, const int32_t* trg_start,
                           const uint64_t* col_off, const uint8_t* trg_cols, const uint8_t* qry_cols, uint8_t want_profile,
                           struct fg_divergence_batch* out);
void fg_release_divergence(struct fg_divergence_batch* b);

/* Trestle's read partitioning (flye/trestle/trestle.py:1075-1142, partition_reads), two calls for batches of jobs; a job
 * is one (repeat, side, iteration).  Both lend the context's device and stream only, use integers only, validate on the
 * host before any device work and leave *out all zero after an error.  Column bytes below 128, case kept, '-' the gap.
 * Offset arrays need not start at zero.  Sub-batches of whole jobs of at most FG_PARTITION_BATCH_COLS (environment,
 * default 2^27) columns plus table cells (below) and, as switches for tests, FG_PARTITION_BATCH_JOBS jobs and
 * FG_PARTITION_TILE columns per tile (a power of two in 64 .. 4096, default 1024); the result depends on none of them.
 * FG_ERR_NOMEM: a job that alone exceeds the budget.  n_jobs = 0 gives an empty batch (every offset array = {0}).
 *
 * fg_confirm_positions = _evaluate_positions (:1360-1473).  Job j has the edges job_edge_off[j] .. job_edge_off[j+1], in
 * the iteration order of cons_aligns; edge e has ONE alignment of its consensus to the template, collapsed by the caller:
 * trg_start, trg_end, qry_start and the columns col_off[e] .. col_off[e+1].  Both shift_gaps passes run first
 * (EdgeAlignment.__init__; see fg_make_bubbles).  The four tentative lists are job j's x_off[j] .. x_off[j+1] of x_pos, in
 * any order, duplicates allowed; a value outside the walked range never matches.  For edge e and position t in
 * [trg_start, trg_end) (the edge is "in alignment"): c = the (t - trg_start)-th non-gap target column, nuc = the query
 * byte at c, qry_ind = qry_start + the non-gap query bytes before c, has_ins = a non-gap query byte strictly between the
 * previous non-gap target column (or the start) and c.  With min_start / max_end / min_end / max_start over the job's
 * edges, a position t of [min_start, max_end) that `total` holds is judged when side = 0 ("in") and t < min_end, or
 * side = 1 ("out") and t >= max_start; otherwise it goes to no list.  Over the edges in alignment, in order: has_ins sets
 * ins and appends qry_ind - 1 to the edge's cons_pos; ref = nuc of the FIRST such edge, never replaced; a later edge with
 * nuc != ref, neither of them 'N', sets del when ref is '-' and sub otherwise.  With any flag t goes to confirmed total,
 * with del or sub every edge in alignment appends its qry_ind (behind its insertion entry), and t goes to confirmed or
 * rejected ins / del / sub by the matching flag where the tentative list holds t; without a flag t goes to rejected total
 * and to the rejected lists whose tentative list holds it.  The eight lists are ascending; cons_pos is ascending in t and
 * may hold duplicates and -1.  The table cells of a job are max_end - min_start.
 * FG_ERR_ARG: NULL out or NULL where something is read; an offset array that decreases; a byte >= 128; side > 1; a job
 * without edges; trg_start < 0; an edge whose non-gap target columns are not trg_end - trg_start. */
struct fg_confirm_batch {
	uint32_t  n_jobs;
	uint32_t  pad_;
	uint64_t  n_edges;
	uint64_t* conf_total_off;     /* n_jobs + 1, likewise the other seven x_off */
	int32_t*  conf_total_pos;
	uint64_t* conf_sub_off;
	int32_t*  conf_sub_pos;
	uint64_t* conf_del_off;
	int32_t*  conf_del_pos;
	uint64_t* conf_ins_off;
	int32_t*  conf_ins_pos;
	uint64_t* rej_total_off;
	int32_t*  rej_total_pos;
	uint64_t* rej_sub_off;
	int32_t*  rej_sub_pos;
	uint64_t* rej_del_off;
	int32_t*  rej_del_pos;
	uint64_t* rej_ins_off;
	int32_t*  rej_ins_pos;
	uint64_t* cons_off;           /* n_edges + 1: edge job_edge_off[0] + i has cons_pos[cons_off[i] .. cons_off[i+1]] */
	int32_t*  cons_pos;
	void*     owner_;
};
int  fg_confirm_positions(fg_ctx* ctx, uint32_t n_jobs, const uint8_t* side, const uint64_t* job_edge_off,
                          const int32_t* trg_start, const int32_t* trg_end, const int32_t* qry_start, const uint64_t* col_off,
                          const uint8_t* trg_cols, const uint8_t* qry_cols, const uint64_t* total_off, const int32_t* total_pos,
                          const uint64_t* sub_off, const int32_t* sub_pos, const uint64_t* del_off, const int32_t* del_pos,
                          const uint64_t* ins_off, const int32_t* ins_pos, struct fg_confirm_batch* out);
void fg_release_confirm(struct fg_confirm_batch* b);

/* fg_classify_reads = _classify_reads with _index_mapping (:1539-1628).  Job j has the edges job_edge_off[j] ..
 * job_edge_off[j+1] in read_aligns order and job_n_reads[j] = len(headers_to_id) reads.  Edge e has its consensus_pos list
 * edge_pos[edge_pos_off[e] .. edge_pos_off[e+1]] (fg_confirm_positions' cons_pos as it is) and the alignments
 * edge_aln_off[e] .. edge_aln_off[e+1] in list order; alignment a has read[a] < n_reads (the caller's number of
 * aln.qry_id; the same number in one job is the same read, across edges), trg_start, trg_end and its columns.  No
 * shift_gaps: the reference scores the parser's strings.  score(a) = the entries p of the edge's list, with multiplicity,
 * with trg_start <= p < trg_end and equal bytes in trg_cols and qry_cols at the (p - trg_start)-th non-gap target column.
 * The reference zeroes read_scores[read][edge] at EVERY alignment and scores a read's first two per edge, so the
 * (read, edge) score is the score of the LAST alignment in list order when the read has one or two on the edge, and 0 with
 * three or more.  The edges a read has an alignment on vote, in edge order:
 *     top_edge = none, top_score = 0, total = 0, tie = false
 *     s - buffer_count > top_score:                         top_edge = edge, top_score = s, tie = false
 *     else s - buffer_count <= top_score and s >= top_score: top_score = s, tie = true
 *     else s >= top_score - buffer_count and s < top_score:  tie = true
 *     total += s
 * status = 0 ("None") without an alignment or with total = 0, else 1 ("Tied") with tie, else 2 ("Partitioned");
 * top_edge = the index within the job, -1 unless status is 2; top_score and total_score as they stand.  want_scores also
 * returns per alignment (from edge_aln_off[job_edge_off[0]] on) aln_score, its own count, and aln_counted, 1 where it is
 * the one whose score its edge keeps.  The table cells of a job: per edge, the span from its alignments' smallest
 * trg_start to their largest trg_end.
 * FG_ERR_ARG: as fg_confirm_positions (an alignment's non-gap target columns against trg_end - trg_start); also
 * read[a] >= n_reads, buffer_count < 0, and a job whose edge lists together hold 2^31 entries or more. */
struct fg_classify_batch {
	uint32_t  n_jobs;
	uint32_t  pad_;
	uint64_t  n_alignments;
	uint64_t* read_off;           /* n_jobs + 1, into the four arrays below */
	uint8_t*  status;             /* 0 None, 1 Tied, 2 Partitioned */
	int32_t*  top_edge;
	int32_t*  top_score;
	int32_t*  total_score;
	int32_t*  aln_score;          /* want_scores: n_alignments */
	uint8_t*  aln_counted;
	void*     owner_;
};
int  fg_classify_reads(fg_ctx* ctx, int32_t buffer_count, uint32_t n_jobs, const uint64_t* job_edge_off, const uint32_t* job_n_reads,
                       const uint64_t* edge_pos_off, const int32_t* edge_pos, const uint64_t* edge_aln_off, const uint32_t* read,
                       const int32_t* trg_start, const int32_t* trg_end, const uint64_t* col_off, const uint8_t* trg_cols,
                       const uint8_t* qry_cols, uint8_t want_scores, struct fg_classify_batch* out);
void fg_release_classify(struct fg_classify_batch* b);

/* fg_expand_cigars(want_cols = 1) followed by fg_divergence_profile as ONE call, with the substitutions of
 * fg_contig_consensus_cigars: contig bytes for contig_len, contig_aln_off for aln_contig, the records (SAM POS, CIGAR
 * runs, SEQ, grouped by contig) for the columns; trg_start = ctg_pos - 1.  Every per-alignment array is indexed by the
 * caller's alignment number and no offset array need start at zero.  Every field of *out equals what the two calls give
 * for the same records; it is released with fg_release_divergence.
 * Sub-batches of whole contigs under FG_DIVERGENCE_BATCH_COLS / FG_DIVERGENCE_BATCH_CONTIGS and the expansion's
 * numbering (2^31 - 1 columns, runs and SEQ bytes, 2^30 - 1 alignments); each sub-batch expands its own alignments
 * (FG_CIGAR_TILE applies, FG_CIGAR_BATCH_COLS and FG_CIGAR_BATCH_ALNS do not); the contig bytes go up once per call.
 * The number of distinct query bytes of the call, which enters every contig's cost, is found from the records before
 * the cut (k_seq_present over the SEQ bytes that M and I runs consume, upper-cased as the expansion stores them, and '-'
 * where a D run has a length): it is the set the columns would show.  Where one sub-batch holds every alignment the SEQ
 * bytes that kernel has read serve the expansion and cross the bus once; otherwise they go up a second time, per
 * sub-batch.  The result depends on none of the switches.
 * Errors: every code of fg_expand_cigars for the same records, then those of fg_divergence_profile that the expansion
 * does not already exclude (FG_ERR_ARG: a threshold that is NaN or negative; a trg_start that is not inside its contig,
 * which only an alignment of insertions alone behind the last base can be; a contig of 2^31 bytes).  FG_ERR_NOMEM: a
 * contig that alone exceeds FG_DIVERGENCE_BATCH_COLS (the same text as fg_divergence_profile's but for the name) or the
 * expansion's numbering.  After an error *out is all zero and the context stays usable.  n_contigs = 0 gives an empty
 * batch. */
int  fg_divergence_profile_cigars(fg_ctx* ctx, double sub_thresh, double del_thresh, double ins_thresh, uint32_t n_contigs,
                                  const uint64_t* contig_off, const uint8_t* contig_seq, const uint64_t* contig_aln_off,
                                  const int32_t* ctg_pos /* SAM POS, 1-based */, const uint64_t* run_off,
                                  const uint8_t* run_op /* ASCII */, const uint32_t* run_len, const uint64_t* read_off,
                                  const uint8_t* read_seq, uint8_t want_profile, struct fg_divergence_batch* out);

/* fg_expand_cigars(want_cols = 1) followed by fg_classify_reads as ONE call.  The jobs, edges, lists and read numbers
 * are those of fg_classify_reads.  The edge consensuses are the contigs of the expansion: edge e has the bytes
 * edge_seq[edge_off[e] .. edge_off[e+1]] (edge_off is indexed by the edge number, from job_edge_off[0] on, like
 * edge_pos_off and edge_aln_off) and its alignments edge_aln_off[e] .. edge_aln_off[e+1] lie on it: the reference aligns
 * each edge's reads to that edge's own consensus.  ctg_pos, run_off, run_op, run_len, read_off and read_seq describe
 * alignment a as for fg_expand_cigars; trg_start = ctg_pos - 1 and trg_end = trg_start + the consensus bytes the runs
 * consume.  Every field of *out equals what the two calls give for the same records; it is released with
 * fg_release_classify.
 * Sub-batches of whole jobs under FG_PARTITION_BATCH_COLS / FG_PARTITION_BATCH_JOBS and the expansion's numbering, as
 * above; FG_PARTITION_TILE and FG_CIGAR_TILE apply.  The edge consensuses go up once per call.
 * Errors: every code of fg_expand_cigars for the records, those of fg_classify_reads for the rest (FG_ERR_ARG:
 * buffer_count < 0, a job without edges, read[a] >= n_reads, edge lists of 2^31 entries); FG_ERR_NOMEM as
 * fg_classify_reads (the same text but for the name) and for a job beyond the expansion's numbering.  After an error
 * *out is all zero and the context stays usable.  n_jobs = 0 gives an empty batch. */
int  fg_classify_reads_cigars(fg_ctx* ctx, int32_t buffer_count, uint32_t n_jobs, const uint64_t* job_edge_off,
                              const uint32_t* job_n_reads, const uint64_t* edge_pos_off, const int32_t* edge_pos,
                              const uint64_t* edge_off, const uint8_t* edge_seq, const uint64_t* edge_aln_off,
                              const uint32_t* read, const int32_t* ctg_pos /* SAM POS, 1-based */, const uint64_t* run_off,
                              const uint8_t* run_op /* ASCII */, const uint32_t* run_len, const uint64_t* read_off,
                              const uint8_t* read_seq, uint8_t want_scores, struct fg_classify_batch* out);

/* The short-plasmid rescue (flye/short_plasmids/, called from flye/main.py after the contigger): the four passes its
 * Python makes over every hit of three PAF files, as integer passes on the device.  The round(cover / length, 3) of
 * calc_mapping_rate, the threshold comparisons, the greedy used_reads filter and the FASTA slices stay with the caller.
 *
 * One hit is one PAF line (flye/utils/sam_parser.py:55-90).  query and target are name ids of ONE name space: the
 * caller numbers the distinct names of the file, queries and targets together, by rank in ascending byte order, so
 * that equal id means equal name and ascending id is the order of sorted(target_hits) (sam_parser.py:102-120).
 * Hits come in file order.  A RUN is a maximal stretch of consecutive hits with one query (a query that comes back
 * later starts a new run, as in read_paf_grouped).  A GROUP is the hits of one run with one target, in file order;
 * groups are numbered run after run and inside a run by ascending target: the order read_paf_grouped yields them in. */
struct fg_paf_hit {
	uint32_t query, target;
	int32_t  query_len, query_start, query_end, target_len, target_start, target_end;
};

/* calc_mapping_rates (unmapped_reads.py:27-61) and the two rates of extract_unique_plasmids (circular_sequences.py:
 * 146-159) before their division: per group the bases unite_mapping_segments leaves on the query side and on the
 * target side.  Over the group's (start, end) pairs sorted by start a segment joins the last united one when start <=
 * last.end (start == last.end + 1 does NOT join) and a united segment counts end - start + 1.  Under the precondition
 * start <= end that is the sum over the sorted segments of max(0, end_i - max(M_i, start_i - 1)), M_i the largest end
 * before segment i (none before the first); the order among equal starts does not matter.  The reference computes
 * something else for end < start, which is why such input is refused.
 * One call is one device batch.  Groups may have any size: up to FG_PAF_WAVE_MAX hits (environment, default and at
 * most 64) a wave takes a group, up to FG_PAF_WG_MAX (default and at most 1024) a workgroup, above that the group's
 * segments are sorted by (group, start) and a segmented running maximum runs over tiles of FG_PAF_TILE segments
 * (64 .. 1024) with a carry from tile to tile.  The three are switches for tests; the result depends on none of them.
 * FG_ERR_ARG, found before any device work: NULL out; NULL hits with n_hits > 0; n_hits > 2^31 - 1; a hit without
 * 0 <= start <= end on either side.  FG_ERR_NOMEM: more than 2^30 - 1 hits (one sort) or device memory.  After an
 * error *out is all zero and the context stays usable.  n_hits = 0 gives an empty batch (group_off = {0}). */
struct fg_paf_group_batch {
	uint64_t  n_hits;
	uint32_t  n_groups;
	uint32_t* order;          /* n_hits: hit indices, group after group, file order inside a group */
	uint64_t* group_off;      /* n_groups + 1 offsets into order */
	uint32_t* group_query;    /* n_groups */
	uint32_t* group_target;   /* n_groups */
	int64_t*  query_cover;    /* n_groups: what calc_mapping_rate sums over the (query_start, query_end) pairs */
	int64_t*  target_cover;   /* n_groups: likewise over (target_start, target_end) */
	void*     owner_;
};
int  fg_paf_groups(fg_ctx* ctx, const struct fg_paf_hit* hits, uint64_t n_hits, struct fg_paf_group_batch* out);
void fg_release_paf_groups(struct fg_paf_group_batch* b);

/* extract_circular_reads (circular_sequences.py:17-44) and the per-group search of extract_circular_pairs (:87-111).
 * The reference's overhangs are 150 (reads) and 300 (pairs).
 * A hit is circular when query == target, query_start < query_end < target_start < target_end, query_start <
 * max_overhang_read and target_len - target_end + 1 < max_overhang_read.  Per query, over the whole file and not per
 * run, the FIRST circular hit with the largest query_end - query_start + 1 is kept (the reference replaces on strict >
 * only).  circ_query / circ_hit list the queries by the index of their first circular hit: the insertion order of the
 * reference's dict, which trim_circular_reads turns into the names circular_read_<i>.
 * The groups are those of fg_paf_groups on the same hits.  For a group with query != target, with
 *   A: query_len - query_end + 1 < max_overhang_pair and target_start < max_overhang_pair
 *   B: query_start < max_overhang_pair and target_len - target_end + 1 < max_overhang_pair
 * pair_first is the first hit of the group in file order with A; pair_second the first hit OTHER than pair_first with
 * B (hits before pair_first, which fail A, are tested; pair_first itself is not); pair_ok is 1 when both exist and
 * mapping_segments_without_intersection (:70-79) holds: second.query_start < second.query_end < first.query_start <
 * first.query_end and first.target_start < first.target_end < second.target_start < second.target_end.  -1 stands for
 * an absent hit; a group with query == target has -1, -1, 0.  The used_reads filter over the groups in order is the
 * caller's.  Overhang sums are formed in 64 bits.
 * Errors as fg_paf_groups.  n_hits = 0 gives an empty batch. */
struct fg_paf_circular_batch {
	uint64_t  n_hits;
	uint32_t  n_circular;
	uint32_t* circ_query;     /* n_circular name ids */
	uint32_t* circ_hit;       /* n_circular hit indices */
	uint32_t  n_groups;
	uint32_t* group_query;    /* n_groups */
	uint32_t* group_target;   /* n_groups */
	int32_t*  pair_first;     /* n_groups: hit index or -1 */
	int32_t*  pair_second;    /* n_groups: hit index or -1 */
	uint8_t*  pair_ok;        /* n_groups */
	void*     owner_;
};
int  fg_paf_circular(fg_ctx* ctx, const struct fg_paf_hit* hits, uint64_t n_hits, int32_t max_overhang_read,
                     int32_t max_overhang_pair, struct fg_paf_circular_batch* out);
void fg_release_paf_circular(struct fg_paf_circular_batch* b);

/* Connected components of an undirected graph: labels[v] (n_vertices entries, the caller's array) = the smallest
 * vertex index of v's component.  Self loops, duplicate edges, n_edges = 0 and isolated vertices are valid input.
 * find_connected_components (flye/short_plasmids/utils.py:7-29) follows from the labels: its DFS numbers the
 * components by ascending smallest member, and a group lists its members ascending, so group[0] is the label.
 * On the device: every edge hooks the larger of its two labels under the smaller (an integer atomic minimum), every
 * vertex then jumps to the root of its label chain; the two repeat until a pass over the edges finds both ends of
 * every edge under one label (the host reads one flag per round).  Labels only decrease and a label never exceeds its
 * vertex, so the rounds end and the result is the same however the atomics interleave.
 * FG_ERR_ARG, found before any device work: NULL labels with n_vertices > 0; NULL edge_u or edge_v with n_edges > 0; a
 * vertex index >= n_vertices.  The context stays usable. */
int  fg_components(fg_ctx* ctx, uint32_t n_vertices, uint64_t n_edges, const uint32_t* edge_u, const uint32_t* edge_v,
                   uint32_t* labels);

/* The tokens of PafHit.__init__ (sam_parser.py:61-72) for a whole PAF buffer; host only, no context.  Lines end at
 * '\n' (a last line need not); the fields of a line are split at runs of the bytes bytes.split() treats as space
 * (' ', '\t', '\n', '\r', '\v', '\f'); fields 0 and 5 are the names, returned as offset and length into text; fields
 * 1-3 and 6-8 are the integers; further fields are ignored.
 * FG_ERR_ARG for NULL out, NULL text with n_bytes > 0, a line with fewer than 9 fields (an empty line included), an
 * integer field that is not an optionally signed decimal number, and a value outside int32.  fg_last_error(NULL) then
 * holds the text, with the 1-based line number, of the calling thread's last failed fg_paf_parse. */
struct fg_paf_text {
	uint64_t  n_hits;
	uint64_t* query_name_off;  uint32_t* query_name_len;
	uint64_t* target_name_off; uint32_t* target_name_len;
	int32_t*  query_len;  int32_t* query_start;  int32_t* query_end;
	int32_t*  target_len; int32_t* target_start; int32_t* target_end;
	void*     owner_;
};
int  fg_paf_parse(const char* text, uint64_t n_bytes, struct fg_paf_text* out);
void fg_release_paf_text(struct fg_paf_text* b);

/* The tokeniser in front of the SAM paths, on the device: what SynchronizedSamReader._read_file_chunk
 * (flye/utils/sam_parser.py:168-213), the per-line part of get_chunk (:355-377) and the expression of :140 make of a
 * whole SAM text, as arrays.  The context lends its device and stream only.  The text goes up once; the host walks none
 * of it.  What needs a dictionary or Python's generator stays with the caller: name lookup, the "Alignment file is not
 * sorted" test over the chunk names, the seeded shuffle, the coverage cut, the sort by read id.
 * Lines: the text is split at 0x0A; the last line may lack it and a final 0x0A starts no further line.  Lines are
 * numbered from 1 over all lines of the text.
 * Records: a line is a record when its first three bytes are none of @PG @HD @SQ @RG @CO (a prefix test: "@PGx" is a
 * header, a line of fewer than three bytes is none) and it holds at least three 0x09.  Every other line is dropped and
 * counts nowhere.  Records come in file order.
 * Chunks: the tab RNAME of a record is the bytes strictly between its second and third tab (may be empty).  A chunk is
 * a maximal run of consecutive records with equal tab RNAME, compared by bytes with the record before, however many
 * dropped lines lie between.
 * Tokens: maximal runs of bytes outside {0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20}, what bytes.strip().split() gives, numbered
 * from 0 in the line; tokens 0 .. 10 matter.  A record with fewer than 11 tokens has status bit 0; it stays a record (it
 * takes part in the reference's shuffle); its token fields, flag, pos and span are 0 and it has no runs.
 * status, per record: bit 0 fewer than 11 tokens; bit 1 FLAG (token 1) / bit 2 POS (token 3) is not of the form
 * [+-]?[0-9]+ or does not fit int32 -- the value is 0 and the caller does what Python's int() does on the bytes; bit 3
 * SEQ (token 9) is the single byte '*'; bit 4 a CIGAR run length beyond uint32 (that run_len is 0).
 * Runs: within CIGAR (token 5) byte i ends a run when it is one of MIDNSHP=X and byte i - 1 is a decimal digit; the
 * length is the value of the maximal digit run that ends at i - 1 (leading zeros allowed); every other byte belongs to
 * no run: re.findall(b"[0-9]+[MIDNSHP=X]"), the tokens of fg_cigar_parse.  N P = X are reported; refusing them stays
 * with fg_expand_cigars.
 * Span: qry_start = hard_left + soft_left and qry_end = (sum of M, I, S) + hard_left - (sum of S - soft_left), with
 * hard_left the first run's length if it is H and soft_left the first non-H run's length if it is S (_parse_cigar
 * :316-320): the coverage cut needs no walk over the runs.
 * All offsets are 64-bit and relative to text; line_len leaves the 0x0A out.
 * The text goes up in sub-batches of whole lines of at most FG_SAM_BATCH_BYTES bytes (environment, default and at most
 * 2^30), found by one backward search for 0x0A from the budget; the device numbers bytes in 32 bits inside one.  It
 * holds 27 words per line of a sub-batch.  FG_SAM_TILE (environment; a power of two in 256 .. 16384, default 4096, other
 * values are rounded down into that set) is the bytes a workgroup takes; a switch for tests.  The result depends on
 * neither.  fg_kernel_times afterwards reports the sums over the sub-batches.
 * FG_ERR_ARG: NULL out; NULL text with n_bytes > 0.  FG_ERR_NOMEM: a line that alone exceeds FG_SAM_BATCH_BYTES (the
 * message names the switch), or device memory.  After an error *out is all zero and the context stays usable.
 * n_bytes = 0 or a text without records gives an empty batch (chunk_off = {0}, run_off = {0}). */
struct fg_sam_text {
	uint64_t  n_lines;         /* all lines of the text, dropped ones included */
	uint64_t  n_records;
	uint64_t  n_chunks;
	uint64_t  n_runs;
	uint64_t* chunk_off;       /* n_chunks + 1 offsets into the records */
	uint64_t* line_no;         /* per record from here on: 1-based */
	uint64_t* line_off;  uint32_t* line_len;
	uint8_t*  status;
	uint64_t* tab_rname_off;   uint32_t* tab_rname_len;
	uint64_t* qname_off;       uint32_t* qname_len;     /* token 0 */
	uint64_t* rname_off;       uint32_t* rname_len;     /* token 2 */
	uint64_t* cigar_off;       uint32_t* cigar_len;     /* token 5 */
	uint64_t* seq_off;         uint32_t* seq_len;       /* token 9 */
	int32_t*  flag;            /* token 1 */
	int32_t*  pos;             /* token 3 */
	int64_t*  qry_start;  int64_t* qry_end;
	uint64_t* run_off;         /* n_records + 1 offsets into the runs */
	uint8_t*  run_op;          /* n_runs, ASCII */
	uint32_t* run_len;         /* n_runs */
	void*     owner_;
};
int  fg_sam_parse(fg_ctx* ctx, const char* text, uint64_t n_bytes, struct fg_sam_text* out);
void fg_release_sam_text(struct fg_sam_text* b);

#ifdef __cplusplus
}
#endif
#endif
