/* Plain-C consumer of the device group (include/flye_gpu.h, fg_group_*): the reads of c_abi_demo.c, the solid k-mer
 * index sharded by target read over the members of one process, and the overlaps of every forward read computed over
 * the shards -- the same lists, in the same order, as fg_overlaps gives on one context.  Build:
 *   cc -std=c99 -Iinclude examples/c_group_demo.c -Lflye_amd/lib -lflyegpu -Wl,-rpath,$PWD/flye_amd/lib -o c_group_demo
 * Run: c_group_demo [device ...]   one member per device named; without arguments two members on device 0 (they
 * share the chip: that exercises the plumbing, not the scaling).
 * Without a GPU it prints the error of fg_group_create and exits with status 2. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "flye_gpu.h"

static uint64_t rng_state = 12345;
static uint32_t rnd(void)
{
	rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
	return (uint32_t)(rng_state >> 33);
}

int main(int argc, char** argv)
{
	enum { GENOME = 30000, NREADS = 60, RLEN = 6000, MAX_MEMBERS = 128 };
	static uint8_t genome[GENOME];
	static uint64_t words[NREADS * ((RLEN + 31) / 32)];
	uint64_t word_off[NREADS + 1];
	int32_t len[NREADS];
	uint32_t ids[NREADS];
	int devices[MAX_MEMBERS] = {0, 0};
	uint32_t n_members = 2, m;
	fg_group* g = NULL;
	struct fg_index_stats st;
	struct fg_group_build_info bi;
	struct fg_group_stats gs;
	struct fg_detector_params p;
	struct fg_overlap_batch b;
	int rc, i, j;

	if (argc > 1)
	{
		n_members = (uint32_t)(argc - 1 < MAX_MEMBERS ? argc - 1 : MAX_MEMBERS);
		for (m = 0; m < n_members; ++m) devices[m] = atoi(argv[m + 1]);
	}
	printf("flye_gpu ABI version %d\n", fg_abi_version());
	rc = fg_group_create(&g, devices, n_members, 17);
	if (rc != FG_OK) { printf("fg_group_create: %s\n", fg_strerror(rc)); return 2; }
	fg_group_size(g, &m);
	printf("group of %u members\n", m);

	for (i = 0; i < GENOME; ++i) genome[i] = (uint8_t)(rnd() & 3);
	memset(words, 0, sizeof(words));
	word_off[0] = 0;
	for (i = 0; i < NREADS; ++i)
	{
		uint32_t start = rnd() % (GENOME - RLEN);
		uint64_t* w = words + word_off[i];
		for (j = 0; j < RLEN; ++j)
		{
			uint8_t base = genome[start + j];
			if (rnd() % 100 < 5) base = (uint8_t)((base + 1 + rnd() % 3) & 3);	/* 5 % substitutions */
			w[j / 32] |= (uint64_t)base << ((j % 32) * 2);
		}
		len[i] = RLEN;
		word_off[i + 1] = word_off[i] + (RLEN + 31) / 32;
		ids[i] = 2u * (uint32_t)i;
	}
	rc = fg_group_set_reads(g, NREADS, words, word_off, len, 0);
	if (rc == FG_OK) rc = fg_group_build_index_solid(g, 2, 0.40f, 100, 100.0f, 1.0f, &st);
	if (rc != FG_OK) { printf("index: %s (%s)\n", fg_strerror(rc), fg_group_last_error(g)); return 1; }
	printf("index: %llu k-mers, %llu entries, repetitive frequency %llu\n", (unsigned long long)st.selected_kmers,
		   (unsigned long long)st.index_entries, (unsigned long long)st.repetitive_frequency);
	fg_group_build_info(g, &bi);
	for (m = 0; m < n_members; ++m)
	{
		uint32_t world = 0, rank = 0;
		uint64_t nk = 0, ne = 0, nr = 0;
		fg_ctx* c = fg_group_member(g, m);		/* borrowed: the group keeps owning it */
		fg_index_shard(c, &world, &rank);
		fg_export_index(c, &nk, &ne, &nr, NULL, NULL, NULL, NULL);
		printf("  member %u on device %d: shard %u of %u, %llu of the entries\n", m, devices[m], rank, world,
			   (unsigned long long)ne);
	}
	printf("  build: %u selection batches, %llu bytes of frequencies and %llu bytes of pieces between members\n",
		   bi.selection_batches, (unsigned long long)bi.freq_bytes, (unsigned long long)bi.scatter_bytes);

	memset(&p, 0, sizeof(p));
	p.max_jump = 1500; p.min_overlap = 1000; p.max_overhang = 1500; p.only_max_ext = 1; p.max_divergence = 1.0f;
	rc = fg_group_overlaps(g, &p, ids, NREADS, 0, 0, &b);
	if (rc != FG_OK) { printf("overlaps: %s (%s)\n", fg_strerror(rc), fg_group_last_error(g)); return 1; }
	printf("%llu overlaps for %u reads, %llu seed hits\n", (unsigned long long)b.n_recs, b.n_queries,
		   (unsigned long long)b.seed_hits);
	for (i = 0; i < 5 && (uint64_t)i < b.n_recs; ++i)
	{
		const struct fg_overlap_rec* r = &b.recs[i];
		printf("%u %d %d %d %u %d %d %d %d %g\n", r->cur_id, r->cur_begin, r->cur_end, r->cur_len, r->ext_id,
			   r->ext_begin, r->ext_end, r->ext_len, r->score, r->seq_divergence);
	}
	fg_group_stats(g, &gs);
	printf("exchange: %llu of %llu seed hits' bytes moved in %llu copies\n", (unsigned long long)gs.hits_moved_bytes,
		   (unsigned long long)(12 * gs.hits_total), (unsigned long long)gs.peer_copies);
	rc = b.n_recs > 0 ? 0 : 1;
	fg_release_batch(&b);
	fg_group_destroy(g);
	return rc;
}
