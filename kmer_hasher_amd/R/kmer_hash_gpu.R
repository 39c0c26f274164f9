## R front-end of the MI355X k-mer position index.
## Same three functions, arguments and results as the reference's index API
## (reference kmer_hash.R:5-28); only the shared object changes: kmer_hash.so is built from
## kmer_hash_glue.c over libkmhgpu.so (see INTEGRATION.md).
local({
    here <- dirname(sys.frame(1)$ofile)
    dyn.load(file.path(here, "kmer_hash.so"))
})

## build the index; positions come back ascending per k-mer whatever do.sort says
make.kmer.hash <- function(seq, k, do.sort=FALSE){
    .Call("make_kmer_h_index", as.character(seq), as.integer(k), as.integer(do.sort))
}

## Not in the reference: an index of the (w,k)-minimizer windows alone (about 2 / (w + 1) of them
## on random sequence); w = 1 .. 256.  Queries on it apply the same rule to the query sequence.
make.kmer.hash.min <- function(seq, k, w, do.sort=FALSE){
    .Call("make_kmer_h_index_min", as.character(seq), as.integer(k), as.integer(w),
          as.integer(do.sort))
}

## opt.flag bits: 1 k-mer strings, 2 (i, pos) rows, 4 (i, x, y) pair rows, 8 counts
kmer.pos <- function(ex.ptr, opt.flag){
    res <- .Call("kmer_positions", ex.ptr, as.integer(opt.flag))
    if(!is.null(res$pos)){
        res$pos <- t(res$pos)
        colnames(res$pos) <- c("i", "pos")
    }
    if(!is.null(res$pair.pos)){
        res$pair.pos <- t(res$pair.pos)
        colnames(res$pair.pos) <- c("i", "x", "y")
    }
    res
}

## dot-plot rows: i = end of the query window, j = start of the indexed occurrence
seq.kmer.pos <- function(ex.ptr, seq, k){
    m <- .Call("sequence_kmer_positions", ex.ptr, as.character(seq), as.integer(k))
    rownames(m) <- c("i", "j")
    t(m)
}

## not in the reference: the dot plot's other strand, seq.kmer.pos(ex.ptr, rc(seq), k) without
## building rc(seq) (the reference's usage script does that on the host with rev.comp /
## reverseComplement).  rc reverses seq and complements each char by its 2-bit code
## ("ACTG"[code ^ 2], rev.comp's rule); one deviation from rev.comp: N stays N (it would become C),
## so N breaks windows on both strands.  Rows are in the coordinates of rc(seq): i = end of the
## window in rc(seq); that window starts at forward position nchar(seq) - i + 1 of seq.
seq.kmer.pos.rc <- function(ex.ptr, seq, k){
    m <- .Call("sequence_kmer_positions_rc", ex.ptr, as.character(seq), as.integer(k))
    rownames(m) <- c("i", "j")
    t(m)
}

## not in the reference: the dot plot as maximal diagonal segments instead of points.  Runs
## seq.kmer.pos (rc=FALSE) or seq.kmer.pos.rc (rc=TRUE) and returns a matrix with columns
## i, j, len, ordered by (i, j): rows (i + t, j + t), t < len, are all in that result and neither
## (i - 1, j - 1) nor (i + len, j + len) is.  len counts windows: the exact match covers
## len + k - 1 bases, drawn with segments(m[,"j"], m[,"i"], m[,"j"] + m[,"len"] - 1,
## m[,"i"] + m[,"len"] - 1).  min.len keeps the segments of at least that many rows; with
## min.len=1 they expand back to exactly seq.kmer.pos's rows.  Position indices only.
seq.kmer.segs <- function(ex.ptr, seq, k, min.len=1, rc=FALSE){
    m <- .Call("sequence_kmer_segments", ex.ptr, as.character(seq), as.integer(k),
               as.integer(min.len), as.integer(rc))
    rownames(m) <- c("i", "j", "len")
    t(m)
}

## row.free=TRUE takes the route that never writes seq.kmer.pos's rows: the same matrix, also
## where the rows are more than 2^31-1 and the function above stops.  The function above stays
## the rows route; the name is bound again to a dispatcher over the two.
.seq.kmer.segs.rows <- seq.kmer.segs
seq.kmer.segs <- function(ex.ptr, seq, k, min.len=1, rc=FALSE, row.free=FALSE){
    if(length(row.free) != 1 || is.na(row.free)) stop("row.free should be TRUE or FALSE")
    if(!row.free) return(.seq.kmer.segs.rows(ex.ptr, seq, k, min.len, rc))
    m <- .Call("sequence_kmer_segments_rf", ex.ptr, as.character(seq), as.integer(k),
               as.integer(min.len), as.integer(rc))
    rownames(m) <- c("i", "j", "len")
    t(m)
}

## not in the reference: seq.kmer.segs' segments merged across small gaps.  On every diagonal,
## neighbouring segments whose gap -- the windows between the end of one and the start of the
## next -- is at most max.gap form one block.  Returns a matrix with columns i, j, span, hits,
## ordered by (i, j): the block starts at row (i, j), spans span windows of its diagonal from its
## first row to its last and holds hits rows of seq.kmer.pos's result (span - hits = the sum of
## its gaps); it covers span + k - 1 bases, drawn with segments(m[,"j"], m[,"i"],
## m[,"j"] + m[,"span"] - 1, m[,"i"] + m[,"span"] - 1).  max.gap=k bridges an isolated
## substitution, which removes k consecutive windows; max.gap=0 gives the segments as
## (i, j, len, len).  min.len drops shorter segments before merging (the gap then spans them),
## min.hits keeps the blocks of at least that many rows.  Position indices only.
seq.kmer.blocks <- function(ex.ptr, seq, k, max.gap=k, min.len=1, min.hits=1, rc=FALSE){
    m <- .Call("sequence_kmer_blocks", ex.ptr, as.character(seq), as.integer(k),
               as.integer(max.gap), as.integer(min.len), as.integer(min.hits), as.integer(rc))
    rownames(m) <- c("i", "j", "span", "hits")
    t(m)
}

## row.free=TRUE: as in seq.kmer.segs.
.seq.kmer.blocks.rows <- seq.kmer.blocks
seq.kmer.blocks <- function(ex.ptr, seq, k, max.gap=k, min.len=1, min.hits=1, rc=FALSE,
                            row.free=FALSE){
    if(length(row.free) != 1 || is.na(row.free)) stop("row.free should be TRUE or FALSE")
    if(!row.free) return(.seq.kmer.blocks.rows(ex.ptr, seq, k, max.gap, min.len, min.hits, rc))
    m <- .Call("sequence_kmer_blocks_rf", ex.ptr, as.character(seq), as.integer(k),
               as.integer(max.gap), as.integer(min.len), as.integer(min.hits), as.integer(rc))
    rownames(m) <- c("i", "j", "span", "hits")
    t(m)
}

## not in the reference: seq.kmer.blocks' blocks linked across diagonals into chains.  An indel
## shifts the diagonal and splits one alignment into several blocks.  Block a may precede block b
## when b starts after a's last row in both coordinates, the larger of the two gaps (in windows) is
## at most max.dist and their difference -- the diagonal shift -- at most max.drift (minimap2's -g
## and -r).  Every block takes its nearest such predecessor, every block keeps the nearest of the
## blocks that chose it, and the links both ends agree on form the chains (greedy nearest-neighbour
## chaining, not minimap2's dynamic program).  Returns a list: chains, a matrix with columns i, j,
## i.end, j.end, hits, blocks, ordered by (i, j); blocks, the matrix seq.kmer.blocks(ex.ptr, seq,
## k, max.gap, min.len, 1, rc, row.free) gives; chain, per block the row of chains it belongs to (0
## where min.hits dropped its chain).  min.hits keeps the chains of at least that many rows.  Draw
## one chain as a polyline through its blocks:
##   r <- seq.kmer.chains(ptr, seq, k); b <- r$blocks[r$chain == 1, , drop=FALSE]
##   lines(c(rbind(b[,"j"], b[,"j"] + b[,"span"] - 1)), c(rbind(b[,"i"], b[,"i"] + b[,"span"] - 1)))
## Position indices only.
seq.kmer.chains <- function(ex.ptr, seq, k, max.dist=5000, max.drift=500, max.gap=k, min.len=1,
                            min.hits=1, rc=FALSE, row.free=FALSE){
    if(length(row.free) != 1 || is.na(row.free)) stop("row.free should be TRUE or FALSE")
    r <- .Call("sequence_kmer_chains", ex.ptr, as.character(seq), as.integer(k),
               as.integer(max.dist), as.integer(max.drift), as.integer(max.gap),
               as.integer(min.len), as.integer(min.hits), as.integer(rc), as.integer(row.free))
    rownames(r$chains) <- c("i", "j", "i.end", "j.end", "hits", "blocks")
    rownames(r$blocks) <- c("i", "j", "span", "hits")
    list(chains=t(r$chains), blocks=t(r$blocks), chain=r$chain)
}

## not in the reference: the dot plot as a binned count matrix, for results too large to hold or
## plot as points.  The rows of seq.kmer.pos (rc=TRUE: of seq.kmer.pos.rc) are counted per cell on
## the device and never written, so the result's size does not depend on the number of hits and
## more than 2^31-1 hits are no obstacle.  bins: the bin count per axis, a scalar or c(i, j);
## i.range / j.range: c(lo, hi), default 1..nchar(seq) and 1..the index's length; per axis the
## bin width is ceiling(range length / bins).  Returns a list: counts, a numeric matrix (a cell
## may exceed .Machine$integer.max) with counts[bi, bj] = the rows with (i - i0) %/% bin_i ==
## bi - 1 and (j - j0) %/% bin_j == bj - 1; i0, j0, bin_i, bin_j; and n_rows, the hit total.
## Draw it with
##   r <- seq.kmer.raster(ptr, seq, k)
##   image(r$j0 + r$bin_j * (0:ncol(r$counts)), r$i0 + r$bin_i * (0:nrow(r$counts)),
##         t(log1p(r$counts)), xlab="index", ylab="seq")
## Position indices only.
seq.kmer.raster <- function(ex.ptr, seq, k, bins=1024, rc=FALSE, i.range=NULL, j.range=NULL){
    .Call("sequence_kmer_raster", ex.ptr, as.character(seq), as.integer(k), as.integer(bins),
          as.integer(rc), if(is.null(i.range)) NULL else as.integer(i.range),
          if(is.null(j.range)) NULL else as.integer(j.range))
}

## shared k-mers of two indices: rows (a, b) = a position in ptr.a with a position in ptr.b
## (the reference's version crashes, test.R:330; this one visits only live k-mers, same k)
kmer.pairs <- function(ptr.a, ptr.b){
    tmp <- t(.Call("kmer_pair_pos", ptr.a, ptr.b))
    colnames(tmp) <- c("a", "b")
    tmp
}

## per-source k-mer counts; params = c(k, source, source_n); kmer.pos / seq.kmer.pos read the
## count vectors of the returned pointer as positions (reference kmer_hash.R:43-46)
count.kmers <- function(seq, params, hash.ptr=NULL){
    params <- as.integer(params)
    .Call("count_kmers", hash.ptr, params, seq)
}

## not in the reference: kmer.pos k-mer order, "first" (default) or "khash" (the reference's
## bucket order: byte-identical kmer.pos output)
kmer.row.order <- function(ex.ptr, order="khash"){
    invisible(.Call("kmer_row_order", ex.ptr, as.character(order)))
}

## not in the reference: the repeat filter of later queries on a position index.  0 (default) is
## off; with max.occ = n a query window whose k-mer occurs at more than n positions of the index
## gives no hit -- as if those rows were deleted from seq.kmer.pos's result -- in seq.kmer.pos,
## seq.kmer.pos.rc, seq.kmer.segs, seq.kmer.blocks, seq.kmer.chains and seq.kmer.raster; n = 1
## keeps unique k-mers only.  kmer.pos and kmer.pairs ignore it.  Returns the previous value.
kmer.max.occ <- function(ex.ptr, max.occ=0){
    invisible(.Call("kmer_max_occ", ex.ptr, as.integer(max.occ)))
}

## not in the reference: every read of a character vector (one read per element) against a
## position index on both strands in one device call.  Columns read, strand, i, j: read is the
## element's number, strand +1 or -1; the rows of read r on strand +1 are exactly
## seq.kmer.pos(ex.ptr, seqs[r], k), those on strand -1 exactly seq.kmer.pos.rc(ex.ptr, seqs[r], k);
## ordered by read, forward before reverse, then (i, j).  A read of at most k bases has no row.
## strand: 0 both, 1 forward, -1 reverse.
reads.kmer.pos <- function(ex.ptr, seqs, k, strand=0){
    m <- .Call("reads_kmer_positions", ex.ptr, as.character(seqs), as.integer(k), as.integer(strand))
    rownames(m) <- c("read", "strand", "i", "j")
    t(m)
}

## not in the reference: where each read of reads.kmer.pos lies.  A row votes for pos = j - i + k,
## the index position of base 1 of the read (strand +1) or of its reverse complement (strand -1),
## possibly <= 0, in the cell (strand, floor(pos / band)).  One row per read: the cell with the
## most votes (ties: forward, then the smaller bin) as strand and pos = bin * band, its votes
## (hits), the most votes among the read's other cells (second) and all of the read's rows (total);
## a read without rows gives zeros.
reads.kmer.vote <- function(ex.ptr, seqs, k, band=64, strand=0){
    m <- .Call("reads_kmer_votes", ex.ptr, as.character(seqs), as.integer(k), as.integer(band),
               as.integer(strand))
    rownames(m) <- c("read", "strand", "pos", "hits", "second", "total")
    t(m)
}

## canonical k-mer counts of a FASTA/FASTQ file (plain or gzip) into a suffix_hash_n pointer;
## params = c(k, prefix_bits, min_q, thread_n, max_reads, max_mem, source_n, source)
## (reference kmer_hash.R:70-73; counted on the GPU, prefix_bits / thread_n / max_mem only
## change the reference's memory layout and threading, not the counts)
count.kmers.fq.sh.rp <- function(fq.file, params, hash.ptr=NULL){
    params <- as.integer(params)
    .Call("count_kmers_fastq_sh_rp", hash.ptr, params, fq.file)
}

## counts_n x nchar(seq) matrix of canonical k-mer counts along seq (reference kmer_hash.R:75-78)
seq.kmer.depth.sh <- function(hash.ptr, seq, k){
    .Call("seq_kmer_depth_sh", hash.ptr, as.character(seq), as.integer(k))
}

## k-mer count spectra per source combination (reference kmer_hash.R:88-91)
kmer.spec.sh.n <- function(ptr, max.count, comb, comb.inner, source.min){
    .Call("kmer_spectrum_suffix_hash_n", ptr, as.integer(max.count),
          as.integer(comb), as.integer(comb.inner), as.integer(source.min))
}

## canonical k-mer counts of a FASTA/FASTQ file into a single suffix_hash pointer
## (reference kmer_hash.R:55-59)
## params: k, report_n, prefix_bits, max memory, min quality, max_read_n
count.kmers.fq.sh <- function(fq.file, params, hash.ptr=NULL){
    params <- as.integer(params)
    .Call("count_kmers_fastq_sh", hash.ptr, params, fq.file);
}

## k-mer count spectrum of a count.kmers.fq.sh pointer (reference kmer_hash.R:89-91)
kmer.spec.sh <- function(ptr, max.count){
    .Call("kmer_spectrum_suffix_hash", ptr, as.integer(max.count))
}
