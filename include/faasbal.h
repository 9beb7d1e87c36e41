/*
 * faasbal.h -- C ABI of the MI355X push balancer (libfaasbal.so).
 *
 * Drop-in boundary for the heartbeat push dispatcher of Distributed-FaaS.
 * The reference has no FFI; its seam is the method level of PushDispatcher
 * (reference task_dispatcher.py).  Each entry point below names the reference
 * code it replaces.  Plain pointers and sizes only; no torch types.
 *
 * One tick = inbound events -> heartbeat purge -> orphan redistribution ->
 * LRU water-filling dispatch.  All calls for one context must
 * come from one thread (the reference loop is single-threaded).  Errors are
 * negative return codes; fb_last_error() gives the message.  No exception
 * crosses the ABI.
 */
#ifndef FAASBAL_H
#define FAASBAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FB_OK 0
#define FB_EINVAL (-1)  /* bad argument or inconsistent state                 */
#define FB_ENOMEM (-2)  /* device or host allocation failed                  */
#define FB_EHIP (-3)    /* HIP runtime error                                  */
#define FB_ERANGE (-4)  /* a fill level beyond the supported round range: the round table has
                         * at most FB_MAX_ROUNDS rows on every context kind.  Any int32 free
                         * count or message value is accepted by fb_load_state / fb_load_shard /
                         * fb_tick_stage, and a tick is exact whenever its fill level L (full
                         * rounds dispatched, fb_tick_result.fill_level) is <= FB_MAX_ROUNDS - 2,
                         * however large the free counts.  A tick that would need more rows
                         * fails its fb_tick_wait with FB_ERANGE: it commits nothing, the
                         * committed state stays readable and unchanged, and the next launch
                         * runs normally.  No call hangs, overflows or allocates a round table
                         * beyond FB_MAX_ROUNDS rows per 256 queue positions.  (Also: the
                         * compact output form past 255 rounds, see fb_set_compact.) */
#define FB_MAX_ROUNDS 4096
#define FB_ENOSPC (-5)  /* in-flight log full                                 */
#define FB_ESTATE (-6)  /* call out of order (e.g. wait without launch): DESIGN.md §5f,
                         * "The life of a tick", has every call at every point of a tick */
#define FB_ERERUN (-7)  /* sharded: the fill level reached the round table; launch the
                         * same tick again (a wider table), exchange, continue, wait */

/* Inbound message kinds (task_dispatcher.py:347-387). */
#define FB_EV_REGISTER 0   /* {"type":"register","data":{"num_processes":n}}   */
#define FB_EV_RECONNECT 1  /* {"type":"reconnect","data":{"free_processes":n}} */
/* (Both overwrite the free count, so they end a drain, FB_EV_DRAIN below: a restarted
 * worker is a fresh worker.) */
#define FB_EV_HEARTBEAT 2  /* {"type":"heartbeat"}                              */
#define FB_EV_RESULT 3     /* {"type":"result", ...}; seq = task's log sequence */
#define FB_EV_OTHER 4      /* any other type: ignored for known workers         */
/* {"type":"leave"}: the worker's goodbye (absent from the reference, whose only way
 * out is an expired heartbeat).  One leave at clock ts from slot s:
 *   - Purge first.  The purge at ts runs before it, as before every message (:390 of
 *     the previous iteration).
 *   - s holds a record: the record is deleted exactly as that purge deletes an
 *     expired one -- the record is gone, the slot is out of the LRU queue, and a
 *     registration that existed at tick start counts as died-at-start: its in-flight
 *     entries (sequence >= its epoch) are this tick's orphans, dispatched first.
 *   - Later messages of s in the same tick meet an unknown identity: a register opens
 *     a new registration (epoch = the log head at tick start), anything else creates
 *     the free = 0 record and is answered with FB_EVS_RECONNECT (:356-358).
 *   - s holds no record at that point (it never had one, it expired at ts, it already
 *     left): nothing happens.  No record is created and no reconnect is asked for --
 *     a goodbye must not create the worker.
 *   - The status is FB_EVS_APPLIED in both cases; val and seq are ignored.
 *   - The evicted list keeps its rule: a slot is listed when it held a record at tick
 *     start or got any message in the tick, and holds no record after the tick.  So a
 *     leave from a slot that never had a record lists that slot -- which is how a host
 *     mirror that gave the sender a slot number gets it back.
 *   - With a finite tte a leave equals overwriting the record's heartbeat with
 *     ts - tte - 1; it is not done that way, and works with tte = +inf too.
 *   - Deque contexts (no liveness, records never deleted) refuse a batch that holds a
 *     leave at stage: FB_EINVAL, "event %d: leave on a deque context", nothing staged. */
#define FB_EV_LEAVE 5
/* (Kind 6 is unassigned and refused as an unknown kind.) */
/* {"type":"drain"} / {"type":"resume"}: the planned shutdown (absent from the reference):
 * "give me no new work, let me finish what I have".  val != 0 drains, val == 0 resumes;
 * seq is ignored.  There is no new persistent state: a draining record is marked in its
 * free count, which every kernel, load, read, snapshot, summary, compaction and reclaim
 * carries as the opaque int32 it always was.  A record is draining iff
 * FB_IS_DRAINING(free); its true free count is free + FB_DRAIN_BIAS.  A result does
 * free += 1 and queues the worker only at free == 1, so a draining worker never comes
 * back into the LRU queue by itself.  One drain at clock ts from slot s:
 *   - Purge first.  The purge at ts runs before it, as before every message.
 *   - s holds no record at that point (it never had one, it expired at ts, it left):
 *     nothing happens.  No record is created and no reconnect is asked for.  The evicted
 *     list keeps its rule: a touched slot without a record after the tick is listed, as
 *     for a leave.
 *   - s holds a record that is not draining, val != 0:
 *     free = min(free, (1 << 29) - 1) - FB_DRAIN_BIAS, and the slot is out of the LRU
 *     queue.  Nothing else changes: the record, its heartbeat (the operator may have sent
 *     the message, not the worker), its epoch and its in-flight entries stay.  It is not a
 *     death: nothing is orphaned.  The clamp keeps an absurd count inside the draining
 *     range (a count above 2^29 - 1 resumes as 2^29 - 1; one below -(1 << 29) already reads
 *     as draining and is outside what this message supports).
 *   - s already draining, val != 0: nothing changes.
 *   - Resume (val == 0) of a draining record: free += FB_DRAIN_BIAS; if that is > 0 the
 *     slot goes to the front of the LRU queue exactly as a reconnect(n > 0) puts it there.
 *     Of a record that is not draining: nothing.
 *   - The status is FB_EVS_APPLIED in every case.
 *   - Later messages of s, in the tick or after it: a result completes its entry, does
 *     free += 1, updates the heartbeat and never queues the slot; a heartbeat is a
 *     heartbeat; register(n) and reconnect(n) overwrite free and so end the drain; an
 *     expired heartbeat or a leave deletes the record as ever, and its live entries are
 *     orphans as ever.
 *   - fb_read_inflight of s is unchanged by a drain or a resume.
 *   - After any tick the committed state is the one fb_load_state installs from
 *     fb_read_state's arrays: the bias travels in free_processes.
 *   - Deque contexts refuse a batch that holds a drain at stage: FB_EINVAL,
 *     "event %d: drain on a deque context", nothing staged. */
#define FB_EV_DRAIN 7
#define FB_DRAIN_BIAS (1 << 30)
#define FB_DRAIN_BELOW (-(1 << 29))
#define FB_IS_DRAINING(free) ((free) < FB_DRAIN_BELOW)

/* Per-event status written by a tick. */
#define FB_EVS_APPLIED 0
#define FB_EVS_RECONNECT 1 /* sender unknown: reply {"type":"reconnect"}, payload dropped (:356-358) */
#define FB_EVS_UNKNOWN 2   /* deque context: result from an id without a record -- the reference
                            * raises KeyError (:291) and its loop dies; here the message is dropped */

typedef struct fb_ctx fb_ctx;

typedef struct fb_tick_result {
    int64_t n_assigned;  /* tasks dispatched this tick: orphans first, then pending       */
    int64_t n_orphans;   /* in-flight tasks of dead registrations, redistributed first    */
    int64_t queue_len;   /* LRU queue (free_workers) length after the tick                */
    int64_t log_head;    /* log length after the tick: task k got sequence log_head_in+k  */
    int32_t n_evicted;   /* worker records deleted by the tick (purge_workers, :241-249)  */
    int32_t fill_level;  /* water-filling rounds completed (L)                            */
    int32_t max_free;    /* largest effective free count in the queue this tick (sharded:
                          * the true count too, although the ranks exchange the counts clamped
                          * to one or two bytes -- except the narrow launches that re-count the
                          * exchanged bytes, more than 16 ranks or more than 256 queue blocks
                          * without exchanged rows, which report at most 255)              */
    int32_t reruns;      /* internal reruns with a wider round table                      */
    int64_t n_local;         /* sharded: tasks dispatched to this rank's workers (else n_assigned) */
    int64_t n_orphans_local; /* sharded: orphans from this rank's log shard (else n_orphans)       */
} fb_tick_result;

/* Device pointers of the context's state (for zero-copy consumers, e.g.
 * torch tensors built from data_ptr).  Valid until the next fb_tick_commit;
 * after a commit, call fb_sync (or fetch the view again) before reading through
 * it, so that the deferred part of the commit has run. */
typedef struct fb_device_view {
    int32_t *free_processes; /* [n_workers]  PushWorker.free_processes (:205), every
                              * free_processes_stride bytes                    */
    double *last_heartbeat;  /* [n_workers]  PushWorker.last_heartbeat (:206), every
                              * last_heartbeat_stride bytes; NaN for empty slots */
    uint8_t *registered;     /* [n_workers]  slot present in self.workers      */
    int32_t *queue;          /* [queue_len]  free_workers in LRU order (:327)  */
    int32_t *log_slot;       /* [log_head]   worker slot per task sequence     */
    int64_t *orphans;        /* last tick's redistributed sequence numbers     */
    int32_t *evicted;        /* last tick's evicted slots                      */
    int32_t n_workers;
    int64_t queue_len, log_head;
    int32_t last_heartbeat_stride; /* bytes between consecutive slots' heartbeats */
    int32_t free_processes_stride; /* bytes between consecutive slots' free counts */
} fb_device_view;

/* Context: owns every device buffer.  device = HIP device ordinal. */
int fb_create(fb_ctx **out, int32_t max_workers, int64_t max_log, int32_t max_events, int device);
int fb_destroy(fb_ctx *ctx);
const char *fb_last_error(const fb_ctx *ctx);

/* Install a worker-table state (replaces building self.workers and the
 * free_workers OrderedDict by hand, task_dispatcher.py:194, :327).
 * queue: slots in LRU order (front first), each registered, no duplicates.
 * log_slot: worker slot per in-flight task sequence number (-1 = completed).
 * What a state must satisfy and what the device receives of it is stated once, for this
 * call and fb_load_shard, in csrc/faasbal_load.h (load_check, load_image): on
 * heartbeat contexts an entry is kept only if its slot holds a record and its sequence is
 * at or above the slot's epoch (load_entry_live), a deque keeps every entry.  A state that
 * fails a condition is refused with FB_EINVAL, the first failing condition in
 * fb_last_error, and nothing changes.  epoch may be NULL (every epoch 0); any other array
 * that is NULL while its count (n_workers, queue_len, log_len) is above zero is refused in
 * the same way; with a count of zero the array is not read and may be NULL. */
int fb_load_state(fb_ctx *ctx, int32_t n_workers, const uint8_t *registered,
                  const int32_t *free_processes, const double *last_heartbeat,
                  const uint32_t *epoch, const int32_t *queue, int64_t queue_len,
                  const int32_t *log_slot, int64_t log_len);

/* Read the committed state back (any pointer may be NULL).  Between a successful
 * fb_tick_wait and its fb_tick_commit, a context that completes log entries in place
 * (deque, sharded, one GPU with more than 128 K workers; see fb_tick_launch) shows the
 * log with the entries the launched tick's results completed already at -1. */
int fb_read_state(fb_ctx *ctx, uint8_t *registered, int32_t *free_processes,
                  double *last_heartbeat, uint32_t *epoch, int32_t *queue, int64_t *queue_len,
                  int32_t *log_slot, int64_t *log_len);

/* One-GPU heartbeat contexts: in-flight log entries per slot of the committed state
 * (n_workers words; build-defined bookkeeping of the redistribution, DESIGN.md §3:
 * the count of the slot's entries that are neither completed nor redistributed). */
int fb_read_inflight(fb_ctx *ctx, uint32_t *inflight);

/* One-GPU contexts (heartbeat and deque), between ticks: renumber the in-flight log densely.
 * Entry q survives iff it is live: log_slot[q] >= 0 and, on heartbeat contexts, its slot holds a
 * record and q >= epoch[slot] (the rule a load applies: load_entry_live, csrc/faasbal_load.h;
 * k_log_normalize's on the device).  Survivors keep their
 * order; new sequence = number of survivors below q.  Every slot's epoch becomes the number of
 * survivors below min(epoch, log_head).  log_head becomes *n_kept.  Nothing else of the committed
 * state changes (records, queue / window, free counts, in-flight counts, round hints), and the
 * tick pipeline keeps its state (a window stays a window).
 * kept_seq (may be NULL; cap entries): old sequence of each new sequence, ascending.
 * expect_kept >= 0: if the live count differs, FB_ESTATE and nothing changes (a host mirror that
 * disagrees).  cap < live count with kept_seq != NULL: FB_EINVAL and nothing changes.
 * FB_ESTATE also: a sharded context (its sequence numbers are global across ranks: compacting
 * them needs a collective), and out of order.  A tick whose fb_tick_wait failed
 * with FB_ENOSPC is discarded (launch it again with the new sequences), as fb_load_state
 * discards it: on every context kind the entries its results named count as live and are kept.
 * Replaces nothing in the reference, which keeps no log (README.md:263-264). */
int fb_log_compact(fb_ctx *ctx, int64_t expect_kept, int64_t *kept_seq, int64_t cap, int64_t *n_kept);

/* Sharded contexts, between ticks: the group's log renumbered densely by two calls per rank
 * around one all-reduce ("A shard group's log"), the shape of a sharded tick.
 *   1. fb_log_compact_shard_mark on every rank: its part of a live bitmap over the global
 *      sequences [0, log_head), one bit per sequence, into device_buffer;
 *   2. the ranks all-reduce (SUM over uint8) the first *bytes bytes: the ranks' sequences are
 *      disjoint, so no byte carries and the sum is the union; they agree on the sum of their
 *      live counts;
 *   3. fb_log_compact_shard_apply on every rank with that sum, or fb_log_compact_shard_cancel
 *      on every rank.
 * fb_log_compact_shard_bytes: *bytes = the bitmap's size, whole tiles of the global head (8 bytes
 * per 64 sequences, a multiple of 256; the same on every rank; 0 for an empty log: nothing to
 * reduce).
 * fb_log_compact_shard_mark: device_buffer is this GPU's memory, 8-byte aligned, bytes >= that
 * size.  Every one of the size's bytes is written (bits at or past log_head: 0).  Bit q is set
 * iff q is the sequence of one of this rank's entries and the entry is live by fb_log_compact's
 * rule (log_slot[i] >= 0 and, where entries of dead registrations may be in the log, the slot
 * holds a record and log_seq[i] >= epoch[slot]: load_entry_live).  *n_live_local: this rank's live entries.  The
 * committed state and the tick pipeline stay as they are.  An uncommitted tick is discarded, as
 * fb_load_shard discards it (a tick waited for and not committed because another rank failed, a
 * tick whose wait failed): its in-place clears are taken back first, so the entries its results
 * named count as live.  FB_ESTATE and nothing changes: a one-GPU context (use fb_log_compact),
 * staged events pending, a tick in flight (phase 1, or launched and not waited for), a mark
 * already made.
 * fb_log_compact_shard_apply, after the buffer was reduced in place: counts the reduced bitmap
 * first (writing only scratch); a count that differs from n_live_global is FB_ESTATE, nothing
 * changes and the mark is dropped; kept_seq != NULL with cap < n_live_global is FB_EINVAL and
 * nothing changes.  Otherwise every live local entry keeps its place in the shard's order and
 * its sequence becomes the number of set bits below it; every own slot's epoch becomes the
 * number of set bits below min(epoch, log_head); log_head becomes n_live_global and the local
 * length this rank's live count (*n_kept_local).  kept_seq (may be NULL; cap entries): the GLOBAL
 * kept list, old sequence of each new sequence, ascending, read off the bitmap (the rank that
 * serves the dispatcher asks for it; no per-entry gather).  Nothing else changes: records, the
 * replicated queue, free counts, the tick pipeline's buffers, the round hint, the bound exchange
 * buffer, the log's address.  FB_ESTATE also: no mark.
 * fb_log_compact_shard_cancel drops a mark (FB_OK without one).
 * Between mark and apply / cancel every call that reads or changes the log or launches a tick is
 * refused with FB_ESTATE.
 * Replaces nothing in the reference, which keeps no log (README.md:263-264). */
int fb_log_compact_shard_bytes(fb_ctx *ctx, int64_t *bytes);
int fb_log_compact_shard_mark(fb_ctx *ctx, void *device_buffer, int64_t bytes, int64_t *n_live_local);
int fb_log_compact_shard_apply(fb_ctx *ctx, int64_t n_live_global, int64_t *kept_seq, int64_t cap,
                               int64_t *n_kept_local);
int fb_log_compact_shard_cancel(fb_ctx *ctx);

/* One-GPU heartbeat contexts (both kinds of clears: with in-flight counts and, past 128 K slots,
 * without), between ticks: take live log entries back from workers that stay registered -- a
 * worker restarted under its identity, a task that hangs while its worker heartbeats on; no
 * purge ever fires for either.  Let B = min(below_seq, log_head).  Entry q is reclaimed iff
 * q < B, it is live by fb_log_compact's rule (log_slot[q] >= 0, its slot holds a record and
 * q >= epoch[slot], load_entry_live: entries that lazy commits left behind are not live), and slot_mask == NULL
 * or slot_mask[log_slot[q]] != 0 (slot_mask: n_workers host bytes).  Sequences ascend with
 * dispatch time, so "dispatched before a clock" is a prefix and "of these workers" a mask.
 * Effect: log_slot[q] = -1 for every reclaimed q; where in-flight counts exist
 * (fb_read_inflight) each slot's count drops by the number of its reclaimed entries while its
 * free count stays, so the slot's budget (free + in flight) goes down with the log.  Nothing
 * else of the committed state changes (records, heartbeats, epochs, free counts, the queue /
 * window, log_head, round hints), and the tick pipeline keeps its state (a window stays a
 * window): the state afterwards is the one fb_load_state installs from fb_read_state's arrays
 * with those entries set to -1.  Hence a later result whose seq names a reclaimed entry is an
 * ordinary result that completes nothing, and a later death of the worker does not list the
 * reclaimed entries among its orphans.
 * seq_out / slot_out (either or both may be NULL; cap entries each): the reclaimed sequences,
 * ascending, and the slot each was on.  *n_reclaimed (may be NULL) is set as soon as the count
 * is known, which is before anything but scratch is written: with an output given and
 * cap < the count, FB_EINVAL, nothing changes and *n_reclaimed holds the count to come back
 * with.  below_seq < 0: FB_EINVAL.
 * FB_ESTATE: a deque context (no liveness), a sharded context (its sequences are global across
 * ranks: a rank's part of its group's reclaim is fb_log_reclaim_shard), and out of order, as
 * fb_pool_stats.
 * Answers what the reference leaves open, which keeps no log: "if something happens with the
 * worker, the task is gone", "if a worker ressucitates" (README.md:263-264). */
int fb_log_reclaim(fb_ctx *ctx, int64_t below_seq, const uint8_t *slot_mask, int64_t *seq_out,
                   int32_t *slot_out, int64_t cap, int64_t *n_reclaimed);

/* Sharded contexts, between ticks: this rank's part of its group's reclaim.
 * Unlike a compaction a reclaim renumbers nothing, so whether an entry goes depends only on what
 * the rank that owns it holds: there is no exchange buffer and no collective on the device.  Let
 * B = min(below_seq, the global log_head).  Local entry i is reclaimed iff log_seq[i] < B, it is
 * live by fb_load_shard's rule (log_slot[i] >= 0 on one of the rank's own slots, and, where
 * lazily kept entries may be in the log, its slot holds a record and log_seq[i] >= epoch[slot]),
 * and slot_mask == NULL or slot_mask[log_slot[i] - slot_base] != 0 (slot_mask: this rank's
 * n_workers host bytes, indexed locally like every array of fb_load_shard).
 * Effect: log_slot[i] = -1 for every reclaimed entry, and nothing else: log_seq, the local
 * length, the global head, records, epochs, free counts, the replicated queue, the round hint,
 * the bound exchange buffer and the tick pipeline stay (sharded contexts keep no in-flight
 * counts).  The state afterwards is the one fb_load_shard installs from the rank's read-back
 * arrays with those entries at -1.
 * seq_out / slot_out (either or both may be NULL; cap entries each): the reclaimed entries'
 * global sequences, ascending, and the global slot each was on.  cap and *n_reclaimed are
 * fb_log_reclaim's: the count is set as soon as it is known, before anything but scratch is
 * written; with an output given and cap < the count, FB_EINVAL, nothing changes and the count
 * comes back.  A group calls every rank with cap = 0 first -- a count, and every refusal a rank
 * has to make, before any rank has taken anything -- and only then with room.
 * below_seq < 0: FB_EINVAL.  FB_ESTATE: a one-GPU context (use fb_log_reclaim), between a
 * compaction's mark and its apply or cancel, and out of order, as fb_pool_stats_shard
 * (DESIGN.md §5f); a launch that fb_tick_wait dropped has its in-place clears taken back first,
 * so the entries its results named count as live. */
int fb_log_reclaim_shard(fb_ctx *ctx, int64_t below_seq, const uint8_t *slot_mask, int64_t *seq_out,
                         int32_t *slot_out, int64_t cap, int64_t *n_reclaimed);

/* One-GPU contexts (heartbeat and deque), between ticks: a summary of the committed worker pool
 * at the clock `now`, computed where the state lives (three launches, a few hundred bytes back;
 * DESIGN.md §5e).  A slot is expired iff it is registered and (now - last_heartbeat) > tte, the
 * tick's own test, so n_expired / inflight_expired / dispatchable are what a tick at the same
 * (now, tte) without messages evicts / redistributes / can place.  A log entry is live by
 * fb_log_compact's rule.  The call reads only: the committed state, the log's lazily kept
 * entries included, and the tick pipeline (window, queue buffers, round hints) stay as they are.
 * age_edges: n_edges (0 .. FB_PS_MAX_EDGES) finite, strictly ascending ages for age_hist.
 * Deque contexts have no liveness: now, tte and the edge values are ignored, n_expired,
 * n_queued_expired and inflight_expired are 0, age_hist is all zero, oldest_hb and newest_hb
 * are NaN, dispatchable is -1, and n_queued counts tokens with repetition.
 * FB_EINVAL: out == NULL, n_edges outside [0, FB_PS_MAX_EDGES], and on heartbeat contexts edges
 * not finite and strictly ascending or a non-finite now or tte.  FB_ESTATE: a sharded context
 * (its pool is the group's, which needs a collective: fb_pool_stats_shard on every rank, then
 * fb_pool_merge), and out of order.  A refused call changes nothing.
 * Replaces nothing in the reference, which keeps no such view: its only look at the pool is
 * the per-worker is_alive walk of purge_workers (task_dispatcher.py:241-249).
 * Draining workers (FB_EV_DRAIN) are counted in free_hist[0] and add nothing to free_total. */
#define FB_PS_FREE_BINS 33
#define FB_PS_MAX_EDGES 15
typedef struct fb_pool_summary {
    int64_t n_slots, n_registered;
    int64_t n_expired;        /* registered and (now - hb) > tte: what a purge at `now` evicts   */
    int64_t n_queued;         /* queue positions (tombstones excluded) whose slot is not expired */
    int64_t n_queued_expired; /* ... whose slot is expired; the two sum to the queue length      */
    int64_t dispatchable;     /* sum of max(free, 1) over the n_queued positions = the tick's
                                 Sigma c; -1 on deque contexts                  */
    int64_t free_total;       /* sum of max(free, 0) over registered, not expired slots          */
    int64_t log_head;
    int64_t inflight;         /* live log entries on slots that are not expired                  */
    int64_t inflight_expired; /* live log entries on expired slots = the orphans of a purge now  */
    int64_t inflight_max;     /* contexts with in-flight counts (fb_read_inflight): the largest
                                 per-slot count over registered slots; else -1                   */
    double oldest_hb, newest_hb; /* min / max heartbeat over registered, not expired slots,
                                 NaN heartbeats skipped; NaN when there is none                  */
    int64_t free_hist[FB_PS_FREE_BINS]; /* registered, not expired: bin clamp(free, 0, 32)       */
    int64_t age_hist[FB_PS_MAX_EDGES + 1]; /* registered: bin = number of edges e with
                                 (now - hb) > e                                                  */
} fb_pool_summary;
int fb_pool_stats(fb_ctx *ctx, double now, double tte, const double *age_edges, int32_t n_edges,
                  fb_pool_summary *out);

/* Sharded contexts, between ticks: this rank's part of the group's pool summary, by the same
 * three launches over its own slots, its log shard and the replicated queue.  In *part:
 * n_slots is the rank's slot count; n_registered, n_expired, free_total, oldest_hb, newest_hb
 * and both histograms cover its own slots; n_queued, n_queued_expired and dispatchable cover
 * the queue positions whose slot is one of its own; inflight and inflight_expired cover its
 * log shard; log_head is the global head; inflight_max is -1 (sharded contexts keep no
 * per-slot counts).  *queue_len is the replicated queue's length.  Arguments are checked as
 * by fb_pool_stats (and queue_len != NULL); the order rules are fb_pool_stats' (DESIGN.md
 * §5f).  FB_ESTATE also: a one-GPU context (use fb_pool_stats). */
int fb_pool_stats_shard(fb_ctx *ctx, double now, double tte, const double *age_edges, int32_t n_edges,
                        fb_pool_summary *part, int64_t *queue_len);
/* Host only, no device work, reads no lifecycle: fold the ranks' parts into the group's
 * summary.  Integer fields and histograms are summed; oldest_hb / newest_hb are the minimum /
 * maximum over the parts that have one (NaN when none has); inflight_max is -1 if any part's
 * is, else the maximum; log_head is the parts' common value.  FB_EINVAL: n_parts < 1, a null
 * pointer, parts that disagree on log_head or on their queue length, or whose queue positions
 * do not sum to it.  ctx may be NULL (then only the code is returned). */
int fb_pool_merge(fb_ctx *ctx, const fb_pool_summary *parts, const int64_t *queue_lens,
                  int32_t n_parts, fb_pool_summary *out);

/* Enqueue one tick on the context's stream (no host sync).
 * Replaces, per tick: the inbound branches (task_dispatcher.py:343-387), the
 * purge (:241-249, called at :390) and the dispatch block (:393-419), plus the
 * build-defined redistribution.  Events are host arrays in arrival order with
 * non-decreasing ts <= now; seq is the log sequence of a result's task or -1.
 * n_pending = tasks waiting in pub/sub (carried-over ones first).
 * Reads the committed state, writes the tick's outputs and the next state into
 * separate buffers: launching again without fb_tick_commit recomputes the same
 * tick (used by the benchmark), and the next launch may carry other messages.  This holds
 * on every context kind.  One-GPU heartbeat contexts of at most 128 K workers leave the log
 * untouched until the commit.  The others (deque, sharded, one GPU with more workers) set
 * the log entries that results complete to -1 in place, at launch, and note them: the
 * next launch first names them again unless the tick was committed, and so does, once a
 * tick's fb_tick_wait has failed (FB_ENOSPC, an invalid message, a refused length), the
 * first call that reads or replaces the committed log (fb_read_state, fb_log_compact,
 * fb_pool_stats, fb_device_view_get).  fb_load_state / fb_load_shard drop the notes with
 * the log they replace. */
int fb_tick_launch(fb_ctx *ctx, double now, double tte, int32_t n_events, const uint8_t *kind,
                   const int32_t *slot, const int32_t *val, const double *ts, const int64_t *seq,
                   int64_t n_pending);

/* The same launch in two steps, so that a host can stage tick t+1's events
 * while the device runs tick t (double-buffered pinned staging):
 * fb_tick_stage validates and copies the events (same rules and errors as
 * fb_tick_launch; no device work), fb_tick_launch_staged enqueues the tick on
 * the staged events with the stage's `now`.  fb_tick_launch = stage + launch.
 * Events already in pinned memory (fb_host_alloc) are copied as they are and, on
 * one-GPU heartbeat contexts, checked by the tick's first kernel instead of the
 * host: an invalid message (slot, kind, timestamp) then fails fb_tick_wait with
 * FB_EINVAL naming it, and nothing is committed.  Arrays in this GPU's memory (all of
 * them; seq may be NULL) are not copied at all: the tick reads them in place and its
 * first kernel checks them the same way (overwriting an invalid message with a harmless
 * one); arrays mixing device and host memory are refused.  Pinned arrays must stay
 * unchanged until their tick was waited for, device arrays until it was committed (a
 * window tick's commit reads the slots of its messages). */
int fb_tick_stage(fb_ctx *ctx, double now, int32_t n_events, const uint8_t *kind, const int32_t *slot,
                  const int32_t *val, const double *ts, const int64_t *seq);
int fb_tick_launch_staged(fb_ctx *ctx, double tte, int64_t n_pending);

/* purge_workers (task_dispatcher.py:241-249, called at :390) on its own: a tick at
 * `now` with no messages and no pending tasks.  Records whose heartbeat expired
 * are deleted (fb_get_evicted) and the in-flight tasks of the dead registrations
 * are reported (fb_get_orphans) but NOT dispatched: the caller keeps them pending
 * (the reference drops them, README.md:263-264).  Then fb_tick_wait / outputs /
 * fb_tick_commit as for any tick (sharded contexts: the exchange all-reduce and
 * fb_tick_continue in between, as for a tick). */
int fb_purge_launch(fb_ctx *ctx, double now, double tte);

/* Wait for the last launched tick; fills *res.  Transparently reruns the tick
 * with a wider round table when free counts exceeded the launch's estimate (a sharded
 * context returns FB_ERERUN instead: relaunch).  The table grows to FB_MAX_ROUNDS rows
 * and no further: a tick whose fill level is <= FB_MAX_ROUNDS - 2 is exact for any int32
 * free counts; one that needs more rows fails with FB_ERANGE (on every rank of a sharded
 * group alike), commits nothing and leaves the committed state as it was -- launch a
 * smaller tick (fewer pending tasks) next. */
int fb_tick_wait(fb_ctx *ctx, fb_tick_result *res);

/* Make the waited tick's post-state the committed state.  On a one-GPU
 * heartbeat context the device part (registered / last_heartbeat / epoch of the
 * slots the tick touched or evicted, orphaned log entries) is deferred: the
 * next launch's first kernel runs it, and any call that reads or replaces
 * state first (fb_read_state, fb_load_state, fb_device_view_get, fb_sync, ...)
 * enqueues it on its own.  Observably the same as an immediate commit. */
int fb_tick_commit(fb_ctx *ctx);

/* Copy outputs of the waited tick to host memory. */
int fb_get_assignments(fb_ctx *ctx, int64_t first, int64_t n, int32_t *dst); /* slot per task k */
int fb_get_orphans(fb_ctx *ctx, int64_t n, int64_t *dst);   /* old sequence numbers, ascending */
int fb_get_evicted(fb_ctx *ctx, int32_t n, int32_t *dst);   /* slots, ascending                */
int fb_get_event_status(fb_ctx *ctx, int32_t n, uint8_t *dst); /* FB_EVS_* per event          */

/* All three of the waited tick's lists (each may be NULL; sizes res->n_assigned,
 * n_orphans, n_evicted) with one synchronisation: into pinned memory, three DMA
 * transfers back to back. */
int fb_get_outputs(fb_ctx *ctx, int32_t *assign, int64_t *orphans, int32_t *evicted);

/* Compact assignments (one-GPU contexts).  After fb_set_compact(ctx, 1) every tick
 * also writes, per position of its LRU order (fronts ++ queue ++ backs, n_pos of them),
 * the slot and min(c, L + 1) of the worker there (c = effective free count, 0 = no live
 * queued worker): with the fill level L this determines every assignment of the tick
 * (task k of round r <= L goes to the (k - S(r))-th position with c > r), in 5 bytes per
 * position instead of 4 per task (configs[2]: 0.3 MB instead of 4.1 MB to read back).
 * fb_get_outputs_compact copies that form plus the orphans and evicted slots with one
 * synchronisation (cap = entries of slot / c; *n_pos = positions written; FB_ERANGE
 * when L + 1 > 255); fb_expand_compact turns it into fb_get_assignments' array on the
 * host (result->n_assigned slots). */
int fb_set_compact(fb_ctx *ctx, int enable);

/* Window ticks (one-GPU heartbeat contexts).  A tick at fill level 0
 * (fewer tasks than live queued workers, the streaming case) serves a prefix of the LRU
 * queue; as a window tick it leaves the rest of the queue where it is and appends the
 * re-queued workers at its tail, so its work is O(tasks + messages) instead of O(queue).
 * Results are identical either way (the closed form of task_dispatcher.py:393-419);
 * a tick that turns out not to qualify is rerun on the general path.  mode: -1 auto
 * (the default: contexts of more than 128K workers, after a level-0 tick), 0 off, 1
 * whenever the last tick was not above level 0 (allocates the window buffers on contexts
 * created without them).  Between ticks only. */
int fb_set_window(fb_ctx *ctx, int mode);
/* Committed window ticks, and launches that fell back to the general path. */
int fb_window_stats(fb_ctx *ctx, int64_t *window_ticks, int64_t *fallbacks);
/* Eager commits (a streaming loop that commits every tick it waits for): a window tick's
 * commit is enqueued right behind it at launch and commits on the device as soon as the
 * tick finishes -- if the tick finished as a window tick; otherwise it commits nothing and
 * fb_tick_wait reruns the tick on the general path as usual.  The host still calls
 * fb_tick_wait and fb_tick_commit (which then only does the host's bookkeeping) before the
 * next launch; a tick so launched cannot be relaunched uncommitted, and state reads
 * between its wait and commit see the committed state.  Default off.  Between ticks only. */
int fb_set_eager_commit(fb_ctx *ctx, int enable);
int fb_get_outputs_compact(fb_ctx *ctx, int32_t *slot, uint8_t *c, int64_t cap, int64_t *n_pos, int64_t *orphans,
                           int32_t *evicted);
int fb_expand_compact(fb_ctx *ctx, const int32_t *slot, const uint8_t *c, int64_t n_pos, int32_t *assign);
/* Pinned buffers (fb_host_alloc) that ticks write their compact outputs into while they
 * run: slot / c per position (cap entries), orphans (ocap), evicted slots (ecap); turns
 * compact mode on.  A fused tick (the configs[2] shape) whose outputs fit leaves them
 * there by the time fb_tick_wait returns, and fb_get_outputs_compact into the same
 * buffers copies nothing; other ticks fill them through fb_get_outputs_compact as
 * usual.  The buffers must not be touched between a launch and its wait.  slot = NULL
 * unregisters. */
int fb_set_compact_out(fb_ctx *ctx, int32_t *slot, uint8_t *c, int64_t cap, int64_t *orphans, int64_t ocap,
                       int32_t *evicted, int64_t ecap);

/* Pinned host memory: fb_get_* copies into it are single DMA transfers on the
 * context stream (the drop-in's readback of a tick's assignments). */
int fb_host_alloc(fb_ctx *ctx, int64_t bytes, void **ptr);
int fb_host_free(fb_ctx *ctx, void *ptr); /* ctx may be NULL (the memory outlives contexts) */

/* launch + wait + copies + commit.  Output arrays may be NULL. */
int fb_tick(fb_ctx *ctx, double now, double tte, int32_t n_events, const uint8_t *kind,
            const int32_t *slot, const int32_t *val, const double *ts, const int64_t *seq,
            int64_t n_pending, fb_tick_result *res, uint8_t *ev_status, int32_t *assign,
            int64_t *orphans, int32_t *evicted);

/* Per-operation forms (one-GPU contexts; each is one synchronous tick and commits).
 *
 * fb_apply_events: the inbound branches (task_dispatcher.py:343-387) for n messages
 *   in arrival order, each after the purge at its own clock (:390), then the purge
 *   after the last message at ts[n-1]; nothing is dispatched.  Records that expired
 *   are evicted (evicted), their in-flight tasks reported (orphans) for the caller to
 *   keep pending; ev_status as fb_get_event_status.
 * fb_purge: purge_workers at `now` (:241-249) = fb_purge_launch + wait + outputs + commit.
 * fb_assign: the dispatch block (:393-419) for n_tasks pending tasks after the purge at
 *   `now` (:390); orphans of that purge first (build-defined), then the tasks; assign
 *   gets res->n_assigned slots (fewer than requested when capacity runs out: the rest
 *   stay pending, as at :393).
 * Output arrays may be NULL; sizes as fb_get_* (res->n_*). */
int fb_apply_events(fb_ctx *ctx, double tte, int32_t n_events, const uint8_t *kind, const int32_t *slot,
                    const int32_t *val, const double *ts, const int64_t *seq, fb_tick_result *res,
                    uint8_t *ev_status, int64_t *orphans, int32_t *evicted);
int fb_purge(fb_ctx *ctx, double now, double tte, fb_tick_result *res, int64_t *orphans, int32_t *evicted);
int fb_assign(fb_ctx *ctx, double now, double tte, int64_t n_tasks, fb_tick_result *res, int32_t *assign,
              int64_t *orphans, int32_t *evicted);

int fb_device_view_get(fb_ctx *ctx, fb_device_view *view);

/* Per-kernel device timing with HIP events on the context stream.
 * enable=1 starts accumulating; fb_timing_read syncs and returns, per kernel
 * name (static strings), total milliseconds and launch counts. */
int fb_timing_enable(fb_ctx *ctx, int enable);
int fb_timing_read(fb_ctx *ctx, int32_t max_kernels, const char **names, double *total_ms,
                   int64_t *launches, int32_t *n_kernels);

/* Timing gate (measurement only): hold=1 enqueues a one-lane kernel that holds the
 * context stream until hold=0 releases it, so the launches queued in between run back
 * to back on the device whatever the host's enqueue pace (the gate opens by itself
 * after 0.5 s).  fb_timing_span syncs and returns the device time from the gate's end
 * to the release point's event, and whether the gate timed out.  Per-kernel times of
 * the gated launches come from fb_timing_read as usual. */
int fb_timing_gate(fb_ctx *ctx, int hold);
int fb_timing_span(fb_ctx *ctx, double *ms, int32_t *timed_out);
/* A marker launch for profiles: the gate kernel, already open (it returns at once), so a
 * kernel trace can cut a benchmark's timed region out of the run. */
int fb_timing_mark(fb_ctx *ctx);

/* Device self-test of the kernels' wave/block scan primitives; *errors = 0 on success. */
int fb_selftest(fb_ctx *ctx, int32_t *errors);

/* Diagnostic: copy up to n words of the in-kernel stamp buffer (written only by
 * builds compiled with -DFAASBAL_STAMPS); *n_total = buffer length in words. */
int fb_debug_read(fb_ctx *ctx, unsigned long long *dst, int64_t n, int64_t *n_total);

/* Test paths: run the launch sequence another table size would take on small
 * (oracle-checkable) inputs.  Results are identical on every path.  name / value:
 *   "plan"        0 auto, 1 the k_plan2 + k_emit2 sequence of large tables, 2 the
 *                 chunked k_emit of round tables wider than 128 rows;
 *   "logscan"     -1 auto, 0 never, 1 the log role as its own k_logscan launch;
 *   "split_slots" -1 auto, 0 never, 1 the slot purge as its own k_slots launch;
 *   "ev_ll"       1 per-slot linked lists (one GPU), 0 the radix sort of messages;
 *   "rs_wide"     1 digits up to 11 bits while a batch has <= 4096 sort tiles, 0 8-bit;
 *   "xplan"       sharded: 1 large queues exchange digit rows scanned by k_xscan, 0 a
 *                 phase-2 k_scan re-counts them;
 *   "gp"          one GPU, large tables: 1 k_emit2 reduces the group rows itself, 0 k_plan2;
 *   "win_direct"  window ticks: 1 k_emit_win chunk = workgroup index when every chunk is
 *                 resident at once, 0 always by ticket;
 *   "fault_qlen"  test hook: the next waited tick reports this queue length (checked and
 *                 refused by fb_tick_wait when it exceeds the buffer; -1 off);
 *   "xself"       sharded xplan: 1 k_emit_shard_xp sums the chunk totals itself (<= 64
 *                 chunks), 0 k_xscan's last workgroup does behind a ticket;
 *   "wfirst"      sharded phase 1: 1 k_scan's log and slot blocks ahead of its queue blocks
 *                 (while the log role is fused into k_scan), 0 queue blocks first;
 *   "cmix"        k_emit2 on unfused ticks: 1 compaction workgroups interleaved with the queue
 *                 blocks, 0 after them;
 *   "wtiles"      slot tiles (256 slots each) per slot-purge workgroup: 0 auto (k_scan: 4 on
 *                 unfused tables, 1 fused; k_ev_apply_ll: 4 from 1024 tiles), or 1, 2, 4
 *                 (k_ev_apply_ll: 2 runs as 1);
 *   "qtiles"      k_scan's queue role on unfused one-GPU tables: 0 auto (four queue blocks
 *                 per workgroup), 1 one;
 *   "xcfirst"     sharded xplan phase 2: 1 k_emit_shard_xp's compaction workgroups first in
 *                 its grid when they are many (default), 0 after the queue workgroups;
 *   "lazy"        one-GPU heartbeat contexts: 1 commits leave the log entries they
 *                 redistributed, every later reader tests liveness (default), 0 commits clear
 *                 them (the entries left so far are cleared first);
 *   "gpcheck"     diagnostic (stamps builds): k_plan2 runs beside a gp tick for comparison.
 * Between ticks only; FB_EINVAL for an unknown name or value. */
int fb_set_path(fb_ctx *ctx, const char *name, int value);

/* Synchronise the context stream (for wall-clock benchmarking). */
int fb_sync(fb_ctx *ctx);

/* Run the context's work on another HIP stream (e.g. the one a collective
 * library uses), or on its own stream again with stream = NULL. */
int fb_set_stream(fb_ctx *ctx, void *stream);

/* One-GPU contexts: slot per task of the waited tick as (task index, slot)
 * pairs, same content as fb_get_assignments.  Sharded contexts: only the tasks
 * given to this rank's workers, in ascending task index. */
int fb_get_local_assignments(fb_ctx *ctx, int64_t first, int64_t n, int64_t *task, int32_t *slot);

/* ---- Dispatcher without heartbeats (PushDispatcher.start, task_dispatcher.py:251-322) ----
 * A deque context runs the start() loop per tick: no liveness, no purge, no
 * orphans (now / tte are unused); the ready queue is a deque that may hold an id
 * several times.  register(n) creates the record and, for n > 0, inserts the id
 * at the left even if it is queued already (:276-281); result adds one free
 * process and appends the id at the right when that makes exactly 1 (:284-295);
 * other kinds are ignored; dispatch pops the left id, decrements its count and
 * re-appends it while the count stays > 0 (:298-322).  Replaces, per tick, the
 * message branches and the dispatch block of many loop iterations.
 * max_tokens = deque capacity (ids counted with repetition); fb_load_state's
 * queue may repeat slots; fb_tick_wait fails with FB_ENOSPC if a tick's deque
 * would outgrow it.  Everything else as for fb_create. */
int fb_create_deque(fb_ctx **out, int32_t max_workers, int64_t max_tokens, int64_t max_log,
                    int32_t max_events, int device);

/* ---- Sharded worker table (one process per GPU) ----
 * Rank r owns the global slots [slot_base, slot_base + n_workers): their
 * records, their in-flight log entries (global sequence numbers ascending) and
 * the dispatch of tasks to them.  The LRU queue order is replicated.  A tick is
 *   fb_tick_launch (every rank gets the same full event batch)
 *   -> all-reduce(SUM, uint8) of the bound exchange buffer over all ranks
 *   -> fb_tick_continue -> fb_tick_wait -> outputs -> fb_tick_commit.
 * The whole-table result equals the one-GPU tick's: the union of the ranks'
 * local assignments is fb_get_assignments; orphans / evicted are per rank
 * (merge for the global lists); event status and queue are global. */
int fb_create_sharded(fb_ctx **out, int32_t max_workers_local, int32_t n_workers_global,
                      int64_t max_log_local, int32_t max_events, int device, int32_t rank, int32_t world);
/* queue: global slots in LRU order; log_slot: global slot per local entry
 * (-1 completed); log_seq: its global sequence number; log_head: global log length.
 * Checked and installed by the statement fb_load_state names (csrc/faasbal_load.h), null
 * arrays included (log_seq with log_len > 0, too); the kinds' differences are listed there. */
int fb_load_shard(fb_ctx *ctx, int32_t slot_base, int32_t n_workers, const uint8_t *registered,
                  const int32_t *free_processes, const double *last_heartbeat, const uint32_t *epoch,
                  const int32_t *queue, int64_t queue_len, const int32_t *log_slot, const uint32_t *log_seq,
                  int64_t log_len, int64_t log_head);
int fb_read_shard_log(fb_ctx *ctx, uint32_t *log_seq, int64_t *log_len, int64_t *log_head);
/* Between ticks: the largest free count any queued worker of the loaded state has (the
 * GLOBAL maximum, the same on every rank), which sizes the next tick's round table.
 * A sharded context cannot take it from its own shard: the exchange layout depends on
 * the table, so every rank must agree.  Without it the first tick after fb_load_shard
 * starts narrow and a wider fill level costs one FB_ERERUN relaunch.  Replaces nothing in
 * the reference (it sizes a buffer, task_dispatcher.py:393-419 has none). */
int fb_set_round_hint(fb_ctx *ctx, int32_t max_free);
/* Sharded, between ticks: on != 0 makes this rank's phase 2 also write the whole tick's
 * task -> slot array (every rank computes the global water-filling anyway), so
 * fb_get_assignments works on it and the host needs no per-task gather from the other
 * ranks (the rank that serves the dispatcher loop turns it on).  Replaces the gather of
 * task_dispatcher.py:409-413's decisions onto the loop's process. */
int fb_set_full_assign(fb_ctx *ctx, int on);
/* Exchange buffer size for a tick of n_events events (n_events < 0: the maximum). */
int fb_exchange_bytes(fb_ctx *ctx, int32_t n_events, int64_t *bytes);
/* Device buffer (same size on every rank) the ranks all-reduce between phases. */
int fb_bind_exchange(fb_ctx *ctx, void *device_buffer, int64_t bytes);
/* Enqueue phase 2 of a sharded tick, after the exchange all-reduce. */
int fb_tick_continue(fb_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* FAASBAL_H */
