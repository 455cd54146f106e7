/*
 * ksched.h -- C ABI of the MI355X-native batched pods x nodes predicate evaluator.
 *
 * This is the drop-in boundary for ONE path of acrlabs/kube-scheduler-rs-reference: the
 * per-pod predicate filter-and-pick.  The reference has no FFI of its own (it is a pure Rust
 * binary), so each entry point below names the reference code whose work it replaces.  All
 * file:line citations are into the reference checkout.
 *
 *   reference                                            replaced by
 *   ---------------------------------------------------  ------------------------------------------
 *   node_store snapshot + per-evaluation LIST            ksched_set_nodes   (columns of `available`)
 *     src/main.rs:56, src/predicates.rs:21-38            ksched_update_nodes (sparse rows, from watch events)
 *   node reflector (src/main.rs:134-139): a node's      ksched_update_node_labels (sparse rows, from node watch events)
 *     labels / taints, src/predicates.rs:28-31, 49-50
 *   successful POST (src/main.rs:94-103) changes the     ksched_apply_bindings_device (the batch's bindings, on the device)
 *     next evaluation's LIST; SubAssign src/util.rs:31-36
 *   can_pod_fit            src/predicates.rs:20-43       KSCHED_FIT   bit of ksched_eval*
 *   does_node_selector_match  src/predicates.rs:45-61    KSCHED_SEL   bit of ksched_eval*
 *   check_node_validity    src/predicates.rs:63-77       feasible = fit AND sel (+ fit mask for the reason)
 *   select_node_for_pod    src/main.rs:49-71             KSCHED_PICK_SAMPLED (injected sample indices), ksched_pick_device
 *   (extension E1, BASELINE.json config 5)               KSCHED_PICK_BESTFIT
 *   (extension E2, BASELINE.json config 5)               KSCHED_TAINT
 *   (extension E3: the batch holds every pod's whole row)  KSCHED_PICK_UNIFORM
 *   (extension E4: ... and the nodes' available resources)  KSCHED_PICK_SPREAD
 *   (extension E5: E4 towards the fullest node)            KSCHED_PICK_PACK
 *   (extension E6: boolean expressions over evaluations,   KSCHED_COMBINE_AND / _OR / _ANDNOT
 *     combined in the caller's mask on the device)
 *   (extension E7: soft constraints -- combine only where   KSCHED_COMBINE_SOFT
 *     the pod keeps a node)
 *   (extension E8: the selector operators Exists, Gt, Lt)   KSCHED_SELOP_EXISTS / _GT / _LT
 *   (extension E9: a selector operator per pod and key)     KSCHED_SELOP_TAGGED, KSCHED_SELTAG_*
 *   (extension E10: ORed selector terms in one tagged call)  KSCHED_SEL_TERMS(t), KSCHED_MAX_TERMS
 *
 * Conventions
 *   - plain C, no C++ or torch types; nothing ever unwinds across this boundary: every failure
 *     is a negative return code (ksched_strerror gives the text).
 *   - all quantities are exact signed 64-bit integers on the canonical domain: CPU in
 *     milli-cores, memory in bytes.  `available` may be negative (src/predicates.rs:37).
 *   - nodes are in canonical order (ascending node name); node index == column index.
 *   - label columns are structure-of-arrays: label_val_ids[k*n + node] is the dictionary id of
 *     the value of key k on that node, 0 = key absent.  Ids are exact (interned), never hashes.
 *     sel_val_ids[k*p + pod]: 0 = pod does not constrain key k, KSCHED_SEL_NEVER = the pod asks
 *     for a value no node carries, otherwise the required id.
 *   - masks are pod-major: row `pod` has ksched_mask_words(n) uint64 words, bit (node % 64) of
 *     word (node / 64); padding bits of the last word are always zero.
 *   - the *_device entry points take device pointers (HBM resident, e.g. torch tensors'
 *     data_ptr()) and a hipStream_t passed as void*; they enqueue and return without syncing.
 *     The host-pointer entry points copy in, run, copy out and synchronise.
 *   - a ksched_ctx is internally serialised by a mutex (host side); use one ctx per device.  Evaluations may be enqueued on
 *     any number of the caller's streams: the library orders them against snapshot changes and against each other's use
 *     of ctx-owned scratch memory with events.  Tell it before a stream is destroyed (ksched_forget_stream).
 *   - the *_device entry points are not meant to be captured into a hipGraph and replayed: an evaluation may allocate scratch on its
 *     first use, and some of its scratch is chosen per CALL on the host (the two-stage best-fit pick rotates over three sets of
 *     hand-over counters, each call zeroing the next call's set instead of paying a memset launch).  What a graph would save -- the
 *     launch gap between consecutive steps -- is what ksched_pipe's "alternate" mode addresses (KSCHED_OPT_PIPE_MODE).
 */
#ifndef KSCHED_H
#define KSCHED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KSCHED_ABI_VERSION 7u

/* at most this many label-key columns per batch */
#define KSCHED_MAX_KEYS 32u
/* reference: const ATTEMPTS: u32 = 5 (src/main.rs:49); the ABI accepts any value up to this */
#define KSCHED_MAX_ATTEMPTS 64u
/* selector id meaning "a value that no node carries" -> never matches */
#define KSCHED_SEL_NEVER 0xFFFFFFFFu

/* return codes */
#define KSCHED_OK 0
#define KSCHED_E_INVAL (-1)       /* bad argument (null pointer, inconsistent sizes, bad flags) */
#define KSCHED_E_NODEVICE (-2)    /* no usable MI355X / HIP device; there is NO CPU fallback */
#define KSCHED_E_HIP (-3)         /* a HIP runtime call failed; see ksched_last_error */
#define KSCHED_E_NOMEM (-4)       /* host or device allocation failed */
#define KSCHED_E_STATE (-5)       /* ksched_set_nodes has not been called */
#define KSCHED_E_UNSUPPORTED (-6) /* request outside what this build supports */
#define KSCHED_E_RCCL (-7)        /* RCCL unavailable or a collective call failed; see ksched_comm_last_error */

/* predicate / output selection flags for ksched_eval* */
#define KSCHED_FIT 0x01u           /* resource fit: req <= available on cpu AND memory */
#define KSCHED_SEL 0x02u           /* nodeSelector exact label match */
#define KSCHED_TAINT 0x04u         /* (taints[n] & ~tolerations[p]) == 0   (extension E2) */
#define KSCHED_PICK_SAMPLED 0x08u  /* first feasible of the injected samples, else -1 */
#define KSCHED_PICK_BESTFIT 0x10u  /* lexicographic min (mem residual, cpu residual, node) (extension E1) */
#define KSCHED_WANT_FIT_MASK 0x20u /* also write the fit-only mask (to rebuild InvalidNodeReason) */
/* KSCHED_PICK_UNIFORM (extension E3): uniformly among the pod's feasible nodes; -1 only when it has none.  At most one KSCHED_PICK_*
 * flag per call.  Added in ABI 7 without a version change and without a new symbol: detect it by this constant and its behaviour.
 *   draw    : ONE injected 32-bit draw per pod, u = samples[pod * attempts + 0], 1 <= attempts <= KSCHED_MAX_ATTEMPTS; the other entries
 *             of the pod's row are not read (the same [p][5] table serves either pick).  Here a draw is a number, not a node index.
 *   result  : c = set bits of the pod's feasible row over nodes [0, n).  c == 0: binding -1.  Otherwise k = (uint64(u) * c) >> 32 and the
 *             binding is the index of the k-th set bit (0-based, ascending node index).
 *   exact   : integer arithmetic only -- same inputs, same bits, on every run.  u = 0 gives the lowest feasible node, u = 0xFFFFFFFF the
 *             highest.  For uniform u every feasible node is chosen with probability floor or ceil of 2^32 / c over 2^32: a bias below c / 2^32.
 *   ignored : bits at or beyond n in a row's last word and the words [W, pitch) are never counted and never chosen -- also in the masks a
 *             caller hands to ksched_pick_device / ksched_pick.
 *   n == 0 gives -1 for every pod; p == 0 is a no-op.
 * Accepted, with identical results, by ksched_eval, ksched_eval_begin / ksched_eval_end, ksched_eval_device, ksched_eval_device_pitched,
 * ksched_pick_device, ksched_pick and ksched_pipe_submit (ksched_summarize* takes no pick flag).  KSCHED_E_INVAL for two pick flags at
 * once, out_binding == NULL, samples == NULL with p > 0, attempts == 0 or above the maximum.  The pick always reads the mask, behind the
 * mask kernel: a request without out_feasible evaluates into the ctx's scratch mask, ksched_pipe_submit takes its
 * split route with events, and KSCHED_OPT_PICK_FROM_MASK / KSCHED_OPT_FUSED_PICK have no effect on it.  ksched_last_pick: "uniform". */
#define KSCHED_PICK_UNIFORM 0x40u
/* KSCHED_PICK_SPREAD (extension E4): the least loaded of d uniformly drawn feasible nodes ("power of d choices"); -1 only when the pod has
 * none.  At most one KSCHED_PICK_* flag per call.  Added in ABI 7 without a version change and without a new symbol: detect it by this
 * constant and its behaviour.
 *   draws      : d = attempts, 1 <= d <= KSCHED_MAX_ATTEMPTS.  ALL d entries of the pod's row are read as 32-bit draws:
 *                u_j = samples[pod * attempts + j].  A draw is a number, not a node index.
 *   candidates : c = set bits of the pod's feasible row over nodes [0, n).  c == 0: binding -1.  Otherwise k_j = (uint64(u_j) * c) >> 32 and
 *                v_j is the index of the pod's k_j-th set bit (0-based, ascending node index) -- exactly KSCHED_PICK_UNIFORM's rule, once per
 *                draw.  Candidates may repeat.
 *   result     : the candidate with the largest signed 64-bit (avail_mem[v], avail_cpu[v]), compared lexicographically, memory first (as in
 *                best fit's key); ties go to the lowest node index.  The result does not depend on the order of the draws.
 *   available  : the snapshot as an evaluation enqueued at that point sees it: a ksched_set_nodes, ksched_update_nodes or
 *                ksched_apply_bindings_device enqueued before the call is visible, a change enqueued after it is not -- also when the call
 *                is ksched_pick_device on a stream of its own.
 *   exact      : integer arithmetic only -- same inputs, same bits, on every run.  Negative `available` is legal and compares as signed.
 *                d = 1 gives, bit for bit, the bindings of KSCHED_PICK_UNIFORM for the same column 0.
 *   ignored    : bits at or beyond n in a row's last word and the words [W, pitch) are never counted and never chosen -- also in the masks a
 *                caller hands to ksched_pick_device / ksched_pick.
 *   n == 0 gives -1 for every pod; p == 0 is a no-op.
 * Accepted, with identical results, by ksched_eval, ksched_eval_begin / ksched_eval_end, ksched_eval_device, ksched_eval_device_pitched,
 * ksched_pick_device, ksched_pick and ksched_pipe_submit (ksched_summarize* takes no pick flag).  Errors as for KSCHED_PICK_UNIFORM:
 * KSCHED_E_INVAL for two pick flags at once, out_binding == NULL, samples == NULL with p > 0, attempts == 0 or above the maximum;
 * KSCHED_E_STATE exactly where the uniform pick returns it.  The plan is the uniform pick's too: the pick always reads the mask, behind the
 * mask kernel; a request without out_feasible evaluates into the ctx's scratch mask; KSCHED_OPT_PICK_FROM_MASK / KSCHED_OPT_FUSED_PICK
 * have no effect on it; ksched_pipe_submit takes its split route with events, and a slot's mask is not overwritten before the slot's spread
 * pick has read it.  ksched_last_pick: "spread". */
#define KSCHED_PICK_SPREAD 0x80u
/* KSCHED_PICK_PACK (extension E5): the tightest of d uniformly drawn feasible nodes -- the spread pick towards the fullest node instead of
 * the emptiest, for a caller that consolidates load; -1 only when the pod has none.  At most one KSCHED_PICK_* flag per call.  Added in
 * ABI 7 without a version change and without a new symbol: detect it by this constant and by KSCHED_E_INVAL from an older library.
 *   draws      : d = attempts, 1 <= d <= KSCHED_MAX_ATTEMPTS.  ALL d entries of the pod's row are read as 32-bit draws:
 *                u_j = samples[pod * attempts + j].  A draw is a number, not a node index.
 *   candidates : c = set bits of the pod's feasible row over nodes [0, n).  c == 0: binding -1.  Otherwise k_j = (uint64(u_j) * c) >> 32 and
 *                v_j is the index of the pod's k_j-th set bit (0-based, ascending node index) -- exactly KSCHED_PICK_UNIFORM's rule, once per
 *                draw.  Candidates may repeat.
 *   result     : the candidate with the SMALLEST signed 64-bit (avail_mem[v], avail_cpu[v]), compared lexicographically, memory first.
 *                This is best fit's key: for a fixed pod the residual orders as `available` does.  Ties go to the lowest node index.  The
 *                result does not depend on the order of the draws.  No request column is read: ksched_pick_device needs no req_mem_bytes.
 *   available  : the snapshot as an evaluation enqueued at that point sees it: a ksched_set_nodes, ksched_update_nodes or
 *                ksched_apply_bindings_device enqueued before the call is visible, a change enqueued after it is not -- also when the call
 *                is ksched_pick_device on a stream of its own.
 *   exact      : integers and comparisons only -- same inputs, same bits, on every run.  Negative `available` is legal and compares as
 *                signed.  d = 1 gives, bit for bit, the bindings of KSCHED_PICK_UNIFORM for the same column 0.
 *   ignored    : bits at or beyond n in a row's last word and the words [W, pitch) are never counted and never chosen -- also in the masks a
 *                caller hands to ksched_pick_device / ksched_pick.
 *   n == 0 gives -1 for every pod; p == 0 is a no-op.
 * Accepted, with identical results, by ksched_eval, ksched_eval_begin / ksched_eval_end, ksched_eval_device, ksched_eval_device_pitched,
 * ksched_pick_device, ksched_pick and ksched_pipe_submit (ksched_summarize* takes no pick flag).  Errors as for KSCHED_PICK_SPREAD:
 * KSCHED_E_INVAL for two pick flags at once, out_binding == NULL, samples == NULL with p > 0, attempts == 0 or above the maximum;
 * KSCHED_E_STATE exactly where the uniform pick returns it.  The plan is the spread pick's too: the pick always reads the mask, behind the
 * mask kernel; a request without out_feasible evaluates into the ctx's scratch mask; KSCHED_OPT_PICK_FROM_MASK / KSCHED_OPT_FUSED_PICK
 * have no effect on it; ksched_pipe_submit takes its split route with events, and a slot's mask is not overwritten before the slot's pack
 * pick has read it.  The best-fit order is neither needed nor rebuilt: after a snapshot change a pack request costs what it cost before.
 * ksched_last_pick: "pack". */
#define KSCHED_PICK_PACK 0x100u
/* The pick flags as sets, derived from the flags above (no new value; a flag list is spelled here and nowhere else):
 *   KSCHED_PICK_ANY    : every pick flag -- a call carries at most one of them;
 *   KSCHED_PICK_DRAWS  : the picks that read `samples` (sampled: node indices; the ranked picks: 32-bit draws);
 *   KSCHED_PICK_RANKED : the ranked picks -- uniform, spread and pack rank a 32-bit draw among the pod's feasible nodes, so they always
 *                        read the mask, behind the mask kernel. */
#define KSCHED_PICK_RANKED (KSCHED_PICK_UNIFORM | KSCHED_PICK_SPREAD | KSCHED_PICK_PACK)
#define KSCHED_PICK_DRAWS (KSCHED_PICK_SAMPLED | KSCHED_PICK_RANKED)
#define KSCHED_PICK_ANY (KSCHED_PICK_BESTFIT | KSCHED_PICK_DRAWS)
/* KSCHED_COMBINE_AND / _OR / _ANDNOT (extension E6): fold this call's evaluation into the mask the caller already holds, on the device.
 * One call of the evaluator answers one conjunction (fit AND nodeSelector AND taints, at most KSCHED_MAX_KEYS label columns); with these
 * flags any boolean expression over evaluations -- a selector with more keys than one call takes, a nodeAffinity term with In {a, b} or
 * NotIn {v}, several nodeSelectorTerms (which Kubernetes ORs), "not on a node that already carries X" -- stays in HBM, and the existing
 * picks finish it.  At most one KSCHED_COMBINE_* flag per call.  Added in ABI 7 without a version change and without a new symbol: detect
 * them by these constants and by KSCHED_E_INVAL from an older library.  (0x1000 is not a flag: callers probe with it for KSCHED_E_INVAL.)
 *   meaning    : feasible(this call) is, bit for bit, what the same call WITHOUT the combine flag would have written: the predicates
 *                selected in `flags` against the current snapshot, predicates not selected treated as true.  out_feasible is read AND
 *                written: it is the caller's mask from earlier calls, and becomes out_feasible OP feasible(this call).  Per pod row the
 *                words [0, W) are combined; bits at or beyond n in the row's last word come out ZERO, whatever the old mask held there;
 *                the words [W, pitch) are never read, and are left untouched or written as zero (the existing rule for padding).
 *   exact      : integer logic only -- same inputs, same bits, on every run.
 *   accepted   : by ksched_eval_device and ksched_eval_device_pitched.  NOT by the host-pointer forms ksched_eval and ksched_eval_begin (a
 *                host mask would first have to travel to the device, which is what the flags exist to avoid), nor by ksched_pipe_submit,
 *                ksched_pick* or ksched_summarize*: all of these answer KSCHED_E_INVAL with nothing enqueued and nothing written.
 *   errors     : KSCHED_E_INVAL with nothing enqueued for two combine flags at once, for out_feasible == NULL, and for KSCHED_WANT_FIT_MASK
 *                or out_fit together with a combine flag.  Everything else follows the plain evaluation: KSCHED_E_STATE before
 *                ksched_set_nodes, p == 0 is a no-op, n == 0 leaves the mask alone (and gives -1 for every pod of a pick).
 *   with a pick: a pick flag in the same call runs BEHIND the combine and reads the COMBINED mask: the bindings are exactly those of
 *                ksched_pick_device on that mask with the pick flag alone and no predicate flag.  In particular the best-fit pick is not
 *                told that the mask includes the resource fit -- under OR and AND-NOT it need not --, so req_mem_bytes is not used to skip
 *                candidates.  KSCHED_OPT_PICK_FROM_MASK and KSCHED_OPT_FUSED_PICK have no effect on a combining call.  ksched_last_pick:
 *                "from-mask" for the sampled and the best-fit pick, the member's name for the ranked picks, "none" without a pick;
 *                ksched_last_kernel: the mask kernel's name, as for a plain call.
 *   ordering   : that of a plain ksched_eval_device on `hip_stream`: a set, update or apply enqueued before the call is visible, one
 *                enqueued after it is not.  The call evaluates into the ctx's scratch mask and holds it under the same rule as a ranked pick
 *                without out_feasible: calls on several streams are ordered against each other by the library.
 *   timing     : KSCHED_OPT_TIMING keeps bracketing the mask kernel only.
 * Recipe -- zone In {a, b} AND disk NotIn {hdd} AND fit, then the spread pick, in four calls on one stream and one mask M:
 *     ksched_eval_device(.., sel: zone = a,   KSCHED_SEL,                                            M, ..)   M  = [zone = a]
 *     ksched_eval_device(.., sel: zone = b,   KSCHED_SEL | KSCHED_COMBINE_OR,                        M, ..)   M |= [zone = b]
 *     ksched_eval_device(.., sel: disk = hdd, KSCHED_SEL | KSCHED_COMBINE_ANDNOT,                    M, ..)   M &= ~[disk = hdd]
 *     ksched_eval_device(.., no selector,     KSCHED_FIT | KSCHED_COMBINE_AND | KSCHED_PICK_SPREAD,  M, .., out_binding, ..)
 * (a node WITHOUT the disk label passes NotIn, as in Kubernetes: it does not carry disk = hdd.) */
#define KSCHED_COMBINE_AND 0x200u    /* out_feasible = out_feasible &  feasible(this call) */
#define KSCHED_COMBINE_OR 0x400u     /* out_feasible = out_feasible |  feasible(this call) */
#define KSCHED_COMBINE_ANDNOT 0x800u /* out_feasible = out_feasible & ~feasible(this call) */
#define KSCHED_COMBINE_ANY (KSCHED_COMBINE_AND | KSCHED_COMBINE_OR | KSCHED_COMBINE_ANDNOT)
/* KSCHED_COMBINE_SOFT (extension E7): a SOFT constraint -- narrow the pod's feasible set by this call's evaluation, unless that would leave
 * it empty.  A modifier of KSCHED_COMBINE_AND or KSCHED_COMBINE_ANDNOT in ksched_eval_device and ksched_eval_device_pitched; not a member of
 * KSCHED_COMBINE_ANY, which stays "the ops".  It is what a preferred node-affinity term, a PreferNoSchedule taint and any rule "prefer X,
 * but never leave the pod unbound for it" mean; the decision is per pod row and needs the whole row, so no sequence of AND / OR / AND-NOT
 * gives it.  Added in ABI 7 without a version change and without a new symbol: detect it by this constant and by KSCHED_E_INVAL from an
 * older library.
 *   meaning    : per pod row, with new = feasible(this call), bit for bit what the call writes without any combine flag, and old' = the
 *                caller's row over the words [0, W) with the bits at or beyond n in the last word cleared:
 *                    r = old' & new (KSCHED_COMBINE_AND)    or    r = old' & ~new (KSCHED_COMBINE_ANDNOT);
 *                if r has at least one set bit the row becomes r (the preference narrows), otherwise it becomes old' (the preference is
 *                dropped for this pod).  So a row that was empty stays empty; a non-empty row never becomes empty; a row whose only set
 *                bits were at or beyond n counts as empty and comes out all zero; bits at or beyond n come out zero in every case.  The
 *                words [W, pitch) are never read, and are left untouched or written as zero.
 *   exact      : integer logic only -- same inputs, same bits, on every run.
 *   errors     : KSCHED_E_INVAL with nothing enqueued and nothing written for KSCHED_COMBINE_SOFT without a combine op; with
 *                KSCHED_COMBINE_OR (OR cannot empty a row, so the modifier would mean nothing); for every refusal of a combining call (two
 *                ops, out_feasible == NULL, KSCHED_WANT_FIT_MASK or out_fit); and for the flag at ksched_eval, ksched_eval_begin,
 *                ksched_pipe_submit, ksched_pick* and ksched_summarize*.
 *   otherwise  : the combining call's contract, unchanged: ordering on `hip_stream`; the evaluation goes into the ctx's scratch mask, held
 *                as by any combining call; a pick flag in the same call runs BEHIND the combine and reads the combined mask, with the
 *                bindings of ksched_pick_device on that mask with the pick flag alone; ksched_last_pick and ksched_last_kernel as for a
 *                combining call; KSCHED_OPT_TIMING brackets the mask kernel only; p == 0 is a no-op, n == 0 leaves the mask alone,
 *                KSCHED_E_STATE before ksched_set_nodes.
 * Recipes, beside the one above.  M is the pod batch's HARD mask, built as today; every soft call is one TIER:
 *   preferred node affinity (preferredDuringSchedulingIgnoredDuringExecution), the term's selector ids in sel_val_ids:
 *     ksched_eval_device(.., sel: the preferred term, KSCHED_SEL | KSCHED_COMBINE_AND | KSCHED_COMBINE_SOFT,    M, ..)   affinity
 *     ksched_eval_device(.., sel: the avoided term,   KSCHED_SEL | KSCHED_COMBINE_ANDNOT | KSCHED_COMBINE_SOFT, M, ..)   anti-affinity
 *     the last call carries the pick flag, or ksched_pick_device(M) follows.
 *   PreferNoSchedule taints: keep the soft taints as further bits of the one taint set.
 *     the hard call passes  tolerations | soft_bits  (a soft taint never filters):          KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT, M
 *     the soft call passes the pod's real tolerations:   KSCHED_TAINT | KSCHED_COMBINE_AND | KSCHED_COMBINE_SOFT, M
 * Several tiers, applied most important first, are LEXICOGRAPHIC: a later tier only chooses among what the earlier ones left, and the order
 * of the calls matters.  Kubernetes' weighted sum of preferred terms is not reproduced. */
#define KSCHED_COMBINE_SOFT 0x2000u /* with KSCHED_COMBINE_AND / _ANDNOT: keep the row as it was where the op would empty it */
/* KSCHED_SELOP_EXISTS / _GT / _LT (extension E8): the selector operators that are not equality.  A plain KSCHED_SEL call answers, per
 * (pod, key), "the node's value id equals this id"; In, NotIn and ORed nodeSelectorTerms are built from such calls (E6).  Exists /
 * DoesNotExist ("the node carries key k, whatever the value") and Gt / Lt on a numeric label are no sequence of equality calls: an OPERATOR
 * CALL -- an evaluation whose flag word carries exactly one KSCHED_SELOP_* flag -- answers one such term, as a mask that the combining
 * calls, the soft modifier and the picks consume like any other.  Added in ABI 7 without a version change and without a new symbol: detect
 * them by these constants and by KSCHED_E_INVAL from an older library.
 *   meaning    : per pod and per key k, with e = sel_val_ids[k*p + pod] and v = label_val_ids[k][node] of the current snapshot:
 *                    e == 0                 the pod does not constrain key k: passes, under every operator;
 *                    e == KSCHED_SEL_NEVER  never passes, under every operator -- an encoder's one way to say "this expression can match
 *                                           nothing" (Gt against a non-integer, say);
 *                    any other e            EXISTS: v != 0;    GT: v != 0 && v > e;    LT: v != 0 && v < e.
 *                The compares are UNSIGNED 32-bit on the ids.  A node without the key (v == 0) fails every constrained key under every
 *                operator: Kubernetes' rule for Gt / Lt on a missing label (a bare v < e would let absent nodes through).  Under EXISTS
 *                the entry's value is not looked at beyond "constrained": any id from 1 to 0xFFFFFFFE says "must carry the key".  The row
 *                is the AND over all keys, over nodes [0, n); bits at or beyond n in the last word are zero; the words [W, pitch) are left
 *                untouched or written as zero.  sel_val_ids == NULL, or a snapshot without keys: no pod constrains anything and every
 *                node passes, as for plain KSCHED_SEL.
 *   ids        : the library compares ids, exactly.  ORDERING the ids of a numeric key is the caller's interning: id = value + 1, say, or
 *                the rank of the value among the key's values -- any map that is monotonic over the values of that key and keeps 0 for
 *                "absent".  The bound of a Gt / Lt expression is interned by the same map (it need not be a value some node carries).
 *   exact      : integer logic only -- same inputs, same bits, on every run.
 *   flags      : KSCHED_SEL is required.  Allowed beside it: ONE KSCHED_SELOP_* flag; optionally one KSCHED_COMBINE_* op, with or without
 *                KSCHED_COMBINE_SOFT, under E6 / E7's own rules; optionally one KSCHED_PICK_* flag.  req_cpu_milli / req_mem_bytes stay
 *                required as in every evaluation and are not read.
 *   errors     : KSCHED_E_INVAL with nothing enqueued and nothing written for two operator flags; for an operator flag without KSCHED_SEL;
 *                and for KSCHED_FIT, KSCHED_TAINT, KSCHED_WANT_FIT_MASK or out_fit in the same call -- fit and taints come from another call
 *                and are combined in, as in the recipe below.  Every refusal of a plain or a combining call stays what it is.
 *   accepted   : by ksched_eval and ksched_eval_begin / ksched_eval_end (without a combine flag, as today) and by ksched_eval_device and
 *                ksched_eval_device_pitched (with or without one).  NOT by ksched_pipe_submit, ksched_pick, ksched_pick_device,
 *                ksched_summarize* or ksched_explain: KSCHED_E_INVAL with nothing enqueued.
 *   with a pick: a pick flag in the same call runs BEHIND the mask -- behind the combine, if there is one -- and reads that mask: the
 *                bindings are exactly those of ksched_pick_device on it with the pick flag alone; best fit is told nothing about the fit.
 *                KSCHED_OPT_PICK_FROM_MASK and KSCHED_OPT_FUSED_PICK have no effect (the combining call's rule).  ksched_last_pick:
 *                "from-mask" for the sampled and the best-fit pick, the member's name for the ranked picks, "none" without a pick.
 *   options    : KSCHED_OPT_KERNEL has no effect on an operator call: the operator kernel is the only form, works on every snapshot,
 *                indexed or not, and never reads the bitmap index.  ksched_last_kernel: "selop".  KSCHED_OPT_TIMING brackets the operator
 *                kernel with stream events, as it does the direct kernel.
 *   otherwise  : the plain evaluation's contract: p == 0 is a no-op, n == 0 leaves the mask alone (and gives -1 for every pod of a pick),
 *                KSCHED_E_STATE before ksched_set_nodes; ordering is that of a plain ksched_eval_device on `hip_stream` -- a
 *                ksched_update_node_labels or ksched_set_nodes enqueued before the call is visible to it, one enqueued after it is not --,
 *                and a combining operator call holds the ctx's scratch mask as any combining call does.
 * Recipe -- gpu Exists AND cores Gt 16 AND zone NotIn {z3} AND fit, then the spread pick, in four calls on one stream and one mask M:
 *     ksched_eval_device(.., sel: gpu = 1 (any non-zero), KSCHED_SEL | KSCHED_SELOP_EXISTS,                      M, ..)   M  = [gpu Exists]
 *     ksched_eval_device(.., sel: cores = id(16),         KSCHED_SEL | KSCHED_SELOP_GT | KSCHED_COMBINE_AND,     M, ..)   M &= [cores > 16]
 *     ksched_eval_device(.., sel: zone = z3,              KSCHED_SEL | KSCHED_COMBINE_ANDNOT,                    M, ..)   M &= ~[zone = z3]
 *     ksched_eval_device(.., no selector,                 KSCHED_FIT | KSCHED_COMBINE_AND | KSCHED_PICK_SPREAD,  M, .., out_binding, ..)
 * DoesNotExist is KSCHED_SEL | KSCHED_SELOP_EXISTS | KSCHED_COMBINE_ANDNOT; a preferred expression adds KSCHED_COMBINE_SOFT. */
#define KSCHED_SELOP_EXISTS 0x4000u /* a constrained key passes where the node carries the key at all */
#define KSCHED_SELOP_GT 0x8000u     /* ... where the node carries the key and its id > the pod's entry */
#define KSCHED_SELOP_LT 0x10000u    /* ... where the node carries the key and its id < the pod's entry */
#define KSCHED_SELOP_ANY (KSCHED_SELOP_EXISTS | KSCHED_SELOP_GT | KSCHED_SELOP_LT)
/* KSCHED_SELOP_TAGGED (extension E9): a selector operator per pod and key.  Under a KSCHED_SELOP_* flag above the operator belongs to the
 * CALL: every constrained entry of every pod is read under it, so a batch in which pod A says `cores Gt 16`, pod B `gpu Exists` and pod C
 * `zone = a` takes one evaluation per operator over the whole pods x nodes rectangle plus the combines, and a negated expression (NotIn,
 * DoesNotExist) takes a call of its own.  Under KSCHED_SELOP_TAGGED the operator is part of the selector ENTRY, and ONE call answers a whole
 * conjunctive matchExpressions term for every pod of a heterogeneous batch: In {one value}, NotIn {one value}, Exists, DoesNotExist, Gt and
 * Lt, mixed across keys.  A modifier of KSCHED_SEL in an evaluation; NOT a member of KSCHED_SELOP_ANY (as KSCHED_COMBINE_SOFT is none of
 * KSCHED_COMBINE_ANY).  Added in ABI 7 without a version change and without a new symbol: detect it by this constant and by
 * KSCHED_E_INVAL from an older library.
 *   entry      : e = sel_val_ids[k*p + pod] is read as tag = e >> KSCHED_SELTAG_SHIFT (3 bits), id = e & KSCHED_SELTAG_ID_MASK (29 bits).
 *   meaning    : per pod and per key k, with v = label_val_ids[k][node], the node's FULL 32-bit id of the current snapshot (v == 0: the
 *                node does not carry the key):
 *                    e == 0                    passes everywhere: the pod does not constrain key k;
 *                    tag KSCHED_SELTAG_EQ      v == id               (so id >= 1; an absent node fails) -- In {one value};
 *                    tag KSCHED_SELTAG_NE      v != id               (an absent node PASSES: Kubernetes' NotIn);
 *                    tag KSCHED_SELTAG_EXISTS  v != 0                (the id field is not looked at);
 *                    tag KSCHED_SELTAG_ABSENT  v == 0                (DoesNotExist; the id field is not looked at);
 *                    tag KSCHED_SELTAG_GT      v != 0 && v > id;
 *                    tag KSCHED_SELTAG_LT      v != 0 && v < id      (id 0 or 1: no node);
 *                    tag 6 or 7                nowhere, whatever the id field holds.
 *                KSCHED_SEL_NEVER (0xFFFFFFFF) is tag 7: it keeps its meaning without a special case.  An entry with tag EQ and id 0 IS the
 *                unconstrained entry 0.  The compares are UNSIGNED 32-bit between the node's WHOLE id and the 29-bit id field: a snapshot
 *                may hold ids at or above 2^29 -- they never equal an entry's id, they pass NE, and they pass GT for every bound --, an
 *                entry cannot name them.  That is the one limit of a tagged call: interned ids must stay below 2^29.
 *                The row is the AND over all keys, over nodes [0, n); bits at or beyond n in the last word are zero -- under NE and ABSENT
 *                too, the first rules of this library that an all-zero padding lane would pass; the words [W, pitch) are left untouched
 *                or written as zero.  sel_val_ids == NULL, or a snapshot without keys: every node passes.
 *   exact      : integer logic only -- same inputs, same bits, on every run.
 *   flags      : KSCHED_SEL is required.  Allowed beside the two: optionally one KSCHED_COMBINE_* op, with or without KSCHED_COMBINE_SOFT,
 *                at the two device-pointer evaluations, under E6 / E7's own rules; optionally one KSCHED_PICK_* flag.  req_cpu_milli /
 *                req_mem_bytes stay required as in every evaluation and are not read.
 *   errors     : KSCHED_E_INVAL with nothing enqueued and nothing written for the flag beside any KSCHED_SELOP_EXISTS / _GT / _LT; without
 *                KSCHED_SEL; and for KSCHED_FIT, KSCHED_TAINT, KSCHED_WANT_FIT_MASK or out_fit in the same call -- fit and taints come from
 *                another call and are combined in.  Every refusal of a plain or a combining call stays what it is.
 *   accepted   : by ksched_eval and ksched_eval_begin / ksched_eval_end (without a combine flag, as today) and by ksched_eval_device and
 *                ksched_eval_device_pitched (with or without one).  NOT by ksched_pipe_submit, ksched_pick, ksched_pick_device,
 *                ksched_summarize* or ksched_explain: KSCHED_E_INVAL with nothing enqueued and nothing written.
 *   with a pick: a pick flag in the same call runs BEHIND the mask -- behind the combine, if there is one -- and reads that mask: the
 *                bindings are exactly those of ksched_pick_device on it with the pick flag alone (an operator call's rule, E8).
 *   options    : KSCHED_OPT_KERNEL has no effect: the tagged kernel is the only form, works on every snapshot, indexed or not, and never
 *                reads the bitmap index.  ksched_last_kernel: "seltag".  KSCHED_OPT_TIMING brackets the kernel with stream events.
 *   otherwise  : an operator call's contract (E8): p == 0 is a no-op, n == 0 leaves the mask alone (and gives -1 for every pod of a pick),
 *                KSCHED_E_STATE before ksched_set_nodes; ordering against ksched_update_node_labels / ksched_set_nodes is that of a plain
 *                evaluation on `hip_stream`; a combining tagged call holds the ctx's scratch mask as any combining call does.
 * Recipes:
 *   - gpu Exists AND cores Gt 16 AND zone NotIn {z3} is ONE row -- gpu: EXISTS, cores: GT id(16), zone: NE z3 -- and ONE call,
 *         ksched_eval_device(.., sel: that row per pod, KSCHED_SEL | KSCHED_SELOP_TAGGED,                        M, ..)   M  = [the term]
 *         ksched_eval_device(.., no selector,           KSCHED_FIT | KSCHED_COMBINE_AND | KSCHED_PICK_SPREAD,    M, .., out_binding, ..)
 *     where E8's recipe above takes three calls for the term, each over every pod.
 *   - In {a, b} is two TERMS of one call under KSCHED_SEL_TERMS (extension E10, below); without the term field it stays two calls under
 *     KSCHED_COMBINE_OR (an entry holds one id).
 *   - A range on one key (Gt 4 AND Lt 16) is two calls under KSCHED_COMBINE_AND: a key has one entry per pod per call. */
#define KSCHED_SELOP_TAGGED 0x40000u /* with KSCHED_SEL alone: every selector entry carries its own operator, tag << 29 | id */
#define KSCHED_SELTAG_SHIFT 29u
#define KSCHED_SELTAG_ID_MASK 0x1FFFFFFFu
#define KSCHED_SELTAG_EQ 0u     /* v == id */
#define KSCHED_SELTAG_NE 1u     /* v != id; an absent node passes */
#define KSCHED_SELTAG_EXISTS 2u /* v != 0 */
#define KSCHED_SELTAG_ABSENT 3u /* v == 0 */
#define KSCHED_SELTAG_GT 4u     /* v != 0 && v > id */
#define KSCHED_SELTAG_LT 5u     /* v != 0 && v < id */

/* KSCHED_SEL_TERMS(t) (extension E10): ORed selector terms in one tagged call.  A tagged call (E9) answers ONE conjunctive matchExpressions
 * term per pod.  Kubernetes' requiredDuringSchedulingIgnoredDuringExecution is a LIST of nodeSelectorTerms that are ORed, and `In {a, b, c}`
 * is an OR as well; with E9 alone each further term or set member is a further tagged call over the whole pods x nodes rectangle under
 * KSCHED_COMBINE_OR, into a second mask that is then ANDed into the caller's.  With a TERM COUNT t in bits 20 .. 23 of the flag word the call
 * takes t tagged rows per pod and writes the OR of the t conjunctions, once.  A modifier of a tagged call, as KSCHED_SELOP_TAGGED is one of
 * KSCHED_SEL.  Added in ABI 7 without a version change and without a new symbol: detect it by these constants and by KSCHED_E_INVAL from an
 * older library.  Field 0 is "no term field": every call means what it means without E10.
 *   layout     : sel_val_ids is [t][n_keys][p]: entry (term, k, pod) at ((term * n_keys) + k) * p + pod; at ksched_eval_begin column
 *                (term, k) starts (term * n_keys + k) * sel_stride entries in.  An entry is E9's, unchanged: tag << 29 | id.  The host-pointer
 *                forms copy t * n_keys * p entries.
 *   meaning    : row(pod) = valid bits AND ( OR over term of ( AND over k of [E9's rule for entry (term, k, pod) and the node's id of key k] ) ).
 *                Bits at or beyond n are zero; the words [W, pitch) are left untouched or written as zero.  A term whose entries are all 0
 *                passes everywhere, so a pod without affinity is all zeros.  A term that must match nothing carries KSCHED_SEL_NEVER (or any
 *                tag-6 / tag-7 entry) in any ONE key: the padding term of a pod with fewer than t terms, and Kubernetes' empty term.
 *                sel_val_ids == NULL, or a snapshot without keys: every node passes.  t = 1 gives, bit for bit, the tagged call's mask.
 *   exact      : integer logic only -- same inputs, same bits, on every run.
 *   flags      : KSCHED_SEL | KSCHED_SELOP_TAGGED are required beside a non-zero field; everything else is a tagged call's contract, word for
 *                word: optionally one KSCHED_COMBINE_* op, with or without KSCHED_COMBINE_SOFT, at the two device-pointer evaluations;
 *                optionally one KSCHED_PICK_* flag, which runs behind the mask (behind the combine, if there is one) and reads it.
 *   errors     : KSCHED_E_INVAL with nothing enqueued and nothing written for a non-zero field without KSCHED_SELOP_TAGGED (hence without
 *                KSCHED_SEL, or beside KSCHED_SELOP_EXISTS / _GT / _LT), and for KSCHED_FIT, KSCHED_TAINT, KSCHED_WANT_FIT_MASK or out_fit
 *                beside it.  Every refusal of a tagged, a plain or a combining call stays what it is.
 *   accepted   : where a tagged call is: ksched_eval, ksched_eval_begin / ksched_eval_end, ksched_eval_device, ksched_eval_device_pitched.
 *                NOT by ksched_pipe_submit, ksched_pick, ksched_pick_device, ksched_summarize* or ksched_explain: KSCHED_E_INVAL.
 *   options    : KSCHED_OPT_KERNEL has no effect.  ksched_last_kernel: "selterms" whenever the field is non-zero, t = 1 included.
 *                KSCHED_OPT_TIMING brackets the kernel with stream events.
 *   otherwise  : a tagged call's contract (E9): p == 0 is a no-op, n == 0 leaves the mask alone (and gives -1 for every pod of a pick),
 *                KSCHED_E_STATE before ksched_set_nodes, the ordering of a plain evaluation on `hip_stream`, the ctx's scratch mask held as
 *                by any combining call.
 *   what a row cannot say: one row holds ONE entry per key, so NotIn {a, b} (two NE entries on one key) and a range (Gt 4 AND Lt 16) stay
 *                two calls under KSCHED_COMBINE_AND / _ANDNOT, as under E9.  In {a, b} AND In {x, y} on two keys is four terms (the product).
 * Recipe -- (zone In {a, b} AND gpu Exists) OR (cores Gt 16), then fit and the spread pick, in TWO calls on one stream and one mask M:
 *     three terms per pod, rows [3][n_keys][p]:   term 0: zone = EQ a, gpu = EXISTS;   term 1: zone = EQ b, gpu = EXISTS;   term 2: cores = GT id(16)
 *     (a pod with fewer terms pads with a term holding KSCHED_SEL_NEVER in one key; a pod without affinity is all zeros)
 *     ksched_eval_device(.., sel: those rows, KSCHED_SEL | KSCHED_SELOP_TAGGED | KSCHED_SEL_TERMS(3),              M, ..)   M  = [the affinity]
 *     ksched_eval_device(.., no selector,     KSCHED_FIT | KSCHED_COMBINE_AND | KSCHED_PICK_SPREAD,                M, .., out_binding, ..)
 *   where E9 takes three tagged calls, two of them under KSCHED_COMBINE_OR into a second mask, and a combine of the two masks.
 *   Cost at 100 000 x 5 000, 8 keys (profiles/selterms_cost.txt): where EVERY pod carries T real terms the one call is NOT
 *   cheaper than that sequence (1128 us against 1081 us at T = 2; 2137 against 2182 us at T = 4): both are bound by the scalar decode of the
 *   constrained entries.  Where one pod in a hundred carries terms and the rest have no affinity it is (401 against 629 us at T = 2, 413
 *   against 1298 us at T = 4): a pod whose row is complete after a term stops there.  What the call gives in both cases: one call, one mask. */
#define KSCHED_SEL_TERMS_SHIFT 20u
#define KSCHED_SEL_TERMS_MASK 0x00F00000u
#define KSCHED_SEL_TERMS(t) ((uint32_t)(t) << KSCHED_SEL_TERMS_SHIFT) /* 1 <= t <= KSCHED_MAX_TERMS */
#define KSCHED_MAX_TERMS 15u

/* InvalidNodeReason, src/predicates.rs:14-18 (variant order kept); 0 = Ok(()) */
#define KSCHED_REASON_OK 0
#define KSCHED_REASON_NOT_ENOUGH_RESOURCES 1
#define KSCHED_REASON_NODE_SELECTOR_MISMATCH 2
#define KSCHED_REASON_TAINT_NOT_TOLERATED 3 /* extension E2 only; never produced without KSCHED_TAINT */

/* kernel selection for ksched_set_option(ctx, KSCHED_OPT_KERNEL, v) */
#define KSCHED_OPT_KERNEL 1
#define KSCHED_KERNEL_AUTO 0
#define KSCHED_KERNEL_DIRECT 1  /* lanes = nodes, compare-is-ballot; always applicable */
#define KSCHED_KERNEL_FUSED 3   /* LDS-resident per-tile bitmap index, one launch: rank search + row AND + store (default when applicable) */
/* KSCHED_OPT_TIMING: N > 0 = every N-th mask kernel launch carries hipEvents on its dispatch (1 = every launch; the events
 * cost ~1.5 us of launch gap each, so a throughput measurement samples with N > 1); 0 = off */
#define KSCHED_OPT_TIMING 2
/* KSCHED_OPT_DEBUG: ablation bits for kernel timing experiments (tools/); any non-zero value makes results invalid */
#define KSCHED_OPT_DEBUG 3
/* (bit 30: ksched_summarize* combines a pod's per-tile counts with atomic adds instead of partial words and a reduce kernel -- the
 * design that lost the measurement, kept for re-measuring it (tools/summary_cost.py); the only debug bit that leaves results valid) */

/* KSCHED_OPT_TRACE: 1 = the fused kernel records per-block phase timestamps (diagnostics; see ksched_trace_read) */
#define KSCHED_OPT_TRACE 4
#define KSCHED_TRACE_WORDS 8u /* uint64 words per block: t_entry, t_staged_issue, t_barrier, t_phase1, t_group0, t_loop_end, t_drained, xcc_id */

/* KSCHED_OPT_PICK_FROM_MASK: 1 = KSCHED_PICK_SAMPLED reads the candidates' bits back from the feasibility mask (after
 * the mask kernel); 0 (default) = it tests the drawn candidates directly from the pod and node columns, as the reference
 * does (src/main.rs:53-66: draw, check_node_validity(pod, candidate)), before and independently of the mask kernel.  Same
 * results either way; a bindings-only request (no output mask) then launches no mask kernel at all.
 * KSCHED_PICK_BESTFIT likewise: 0 (default) = candidates are tested in best-fit order from node columns kept in that
 * order, the mask row is only scanned for pods whose best node sits deep in the order; 1 = every candidate's bit is
 * looked up in the mask. */
#define KSCHED_OPT_PICK_FROM_MASK 5
/* KSCHED_OPT_INDEX_BUILD: how ksched_set_nodes fills the per-tile bitmap index: 0 (default) = HIP kernels from the columns in
 * HBM; 1 = the host code that specifies it (csrc/tile_index.hpp), uploaded.  Same tables bit for bit (ksched_index_checksum). */
#define KSCHED_OPT_INDEX_BUILD 6
/* KSCHED_OPT_BESTFIT_STAGES: the best-fit pick from the bitmaps in best-fit order runs in one stage (a wave per pod) or in two
 * (a lane per pod decides from the first 512 - 1024 candidates, a wave per pod finishes the rest): 0 (default) = two stages from
 * 24576 pods per call on (two dependent launches cost ~45 us whatever the batch; one stage ~20 us + 1 us per 1000 pods), 1 = always
 * one, 2 = always two.  Same bindings either way. */
#define KSCHED_OPT_BESTFIT_STAGES 7
/* KSCHED_OPT_SNAPSHOT_STREAM: where ksched_set_nodes / ksched_update_nodes (and the lazy best-fit rebuild) enqueue their device
 * work.  0 (default) = when evaluations have been enqueued on exactly ONE caller stream so far, onto that stream: the change is
 * ordered behind the evaluations already there and ahead of the next ones by the stream itself, with no event and no
 * cross-stream wait (a scheduler loop "pod events -> update -> evaluate" on one stream then never leaves it); with no or several
 * caller streams, onto the ctx's own stream, ordered against the callers' streams by events.  1 = always the ctx's own stream.
 * Same results either way: every evaluation sees the snapshot that was current when it was enqueued. */
#define KSCHED_OPT_SNAPSHOT_STREAM 8
/* KSCHED_OPT_FUSED_PICK: 1 (default) = when an evaluation asks for the feasibility mask AND the sampled pick and the fused mask
 * kernel runs, the pick rides in that launch (select_node_for_pod, src/main.rs:51-71): ONE kernel per step -- as long as the launch
 * is short enough for the pick to hide in its fill (a wave of the kernel has at most five rounds of 64 pods: up to 261 000 pods
 * against 5 000 nodes, 128 000 against 10 000); longer launches keep the pick as its own launch, which is cheaper there.  Two forms,
 * chosen by the request: tile tests -- every block tests the drawn candidates that lie in its own tile against the bitmap rows it
 * holds in LDS, the blocks of a pod combine through one atomic per eight pods (ATTEMPTS = 5 draws, no taint predicate, at most eight
 * label keys) -- or, otherwise, a few waves of every block test the pods' candidates from the node records while the block's tile is
 * staged.  0 = the pick is its own launch ahead of the mask kernel (k_select_sampled); 2 = rides, always as waves of the fill;
 * 3 = rides as tile tests or the call fails with KSCHED_E_UNSUPPORTED (2 and 3: whatever the launch's length).  Same bindings in every form. */
#define KSCHED_OPT_FUSED_PICK 9
/* KSCHED_OPT_FAULT: test hook for the "nothing unwinds across this boundary" rule.  value = kind | (skip << 8): after `skip`
 * further fault points (the places where a call enters the library's C++: snapshot calls, evaluations, explain, checksum) the
 * next one throws inside the call -- kind 1: std::bad_alloc, kind 2: std::runtime_error -- once.  That call must come back with
 * KSCHED_E_NOMEM / KSCHED_E_INVAL and ksched_last_error set; the process must not terminate.  0 = off (default). */
#define KSCHED_OPT_FAULT 10
/* KSCHED_OPT_PIPE_MODE: how ksched_pipe_submit spreads a batch over the pipe's streams.  0 (default) = split: the mask kernel
 * on the mask stream, the pick (and whatever the caller enqueues behind it, e.g. the all-gather of the bindings) on the pick
 * stream.  m >= 1 = alternate: the WHOLE evaluation of a slot -- one launch when the pick rides in the mask kernel -- goes onto
 * stream (slot mod k), k = max(2, m) <= KSCHED_PIPE_MAX_STREAMS: consecutive batches overlap (the next launch's blocks fill while
 * the previous one's blocks still store -- as far as the chip has room for them: KSCHED_OPT_GRID_CUS).  Same results either way;
 * in every mode, and across a change of mode, a slot's mask kernel runs behind the slot's previous mask kernel, its pick behind the
 * slot's previous pick, and a slot's mask is not overwritten by a later submit before the slot's previous pick, where that pick
 * reads the mask (the uniform, the spread and the pack pick always do), has run.  ksched_pipe_wait / ksched_pipe_wait_mask order a consumer behind the slot's work, ksched_pipe_slot_stream names its stream. */
#define KSCHED_OPT_PIPE_MODE 11
#define KSCHED_PIPE_MAX_STREAMS 8u
/* KSCHED_OPT_GRID_CUS: how many of the chip's 256 compute units ONE fused mask launch may occupy (0, the default, = all of them;
 * else 8 .. 256).  A block of the fused kernel owns a compute unit (its tile index fills the LDS), and every block of a launch
 * spends the first microseconds filling it while nothing can be stored; a launch that takes the whole chip leaves no room for
 * the next batch's launch to do that in the meantime.  With the launches of k batches in flight on k streams (the pipe's
 * alternate mode) and 256 / k compute units each, one batch's fill hides under the others' stores.  A throughput setting:
 * a single batch's own latency grows.  Results do not depend on it. */
#define KSCHED_OPT_GRID_CUS 12
/* KSCHED_OPT_MASK_PROBE: candidates ksched_mask_alloc's probe-and-keep path allocates and times (1 .. 16, default 6; 1 = no probing). */
#define KSCHED_OPT_MASK_PROBE 13
/* KSCHED_OPT_ROUND_ORDER: which pods the fused mask kernel's waves take in which order.  A launch cuts the batch into rounds of 64 pods and has
 * chunks * 16 waves per tile working at once.  0 (default) = interleaved, wave-major: round g goes to stream g mod (chunks * 16), neighbouring
 * rounds to different blocks -- the chip writes one moving window of the mask; 2 = interleaved, chunk-major (a block's 16 waves take 16
 * neighbouring rounds); 1 = blocked: every wave owns one contiguous pod range (rounds 1 .. 5's order: chunks * 16 write streams megabytes apart).
 * Results do not depend on it (tests/test_gpu_fullsize.py runs all three); rates do: profiles/r06_round_order.md. */
#define KSCHED_OPT_ROUND_ORDER 14

typedef struct ksched_ctx ksched_ctx;

/* ---- lifetime -------------------------------------------------------------------------- */

/* Create an evaluator bound to HIP device `device_id`.  Fails with KSCHED_E_NODEVICE when the
 * process sees no GPU: the product path has no CPU backend by design. */
int ksched_create(ksched_ctx **out, int device_id);
void ksched_destroy(ksched_ctx *ctx);

uint32_t ksched_abi_version(void);
/* HIP devices the process sees (0 when there is none or the runtime cannot be initialised): what a host checks $KSCHED_DEVICES against */
int ksched_device_count(void);
const char *ksched_strerror(int code);
/* text of the last HIP failure on this ctx (empty string if none); valid until the next call */
const char *ksched_last_error(const ksched_ctx *ctx);
/* words per mask row for n nodes = ceil(n / 64) */
uint32_t ksched_mask_words(uint32_t n_nodes);
int ksched_set_option(ksched_ctx *ctx, int option, int64_t value);

/* ---- node snapshot ----------------------------------------------------------------------
 * Replaces, for a whole batch, what can_pod_fit recomputes per evaluation
 * (src/predicates.rs:27-38): available[n] = allocatable[n] - sum(requests of pods bound to n).
 * Host pointers; the library copies them (they may be reused when the call returns) and builds its device-side indexes with
 * HIP kernels; the call does not wait for the device.  Evaluations already enqueued keep reading the previous snapshot;
 * evaluations enqueued afterwards (on any stream) are ordered behind the build -- by the stream itself when the build rides the
 * one caller stream this ctx has seen, by events otherwise (KSCHED_OPT_SNAPSHOT_STREAM).
 *   avail_cpu_milli, avail_mem_bytes : [n] signed
 *   label_val_ids : [n_keys][n] or NULL when n_keys == 0; ids must be < KSCHED_SEL_NEVER
 *   taints        : [n] bit set of (interned) taints, or NULL = no taints
 */
int ksched_set_nodes(ksched_ctx *ctx, uint32_t n, const int64_t *avail_cpu_milli, const int64_t *avail_mem_bytes,
                     const uint32_t *label_val_ids, uint32_t n_keys, const uint64_t *taints);

/* Incremental form of the same step: `available` of `count` nodes changed -- a pod was
 * bound to or removed from them (src/predicates.rs:36-38 subtracts every pod the LIST returns; here the caller
 * keeps that sum current from watch events instead of re-LISTing).  node_index[i] is a canonical node index
 * (< ksched_num_nodes); the two value arrays hold the node's NEW available cpu / memory.  Labels and taints are
 * not touched (use ksched_update_node_labels when a node's labels or taints change, ksched_set_nodes when the node set
 * changes).  A node listed twice takes its last values.
 * Cost: the new values are scattered into the columns and the fit part (rows, search trees, cnt tables) of the touched
 * 1024-node tiles is rebuilt by one kernel; updates of up to 16 nodes travel in kernel arguments (no copy).  The best-fit
 * order is only marked stale: the next KSCHED_PICK_BESTFIT request rebuilds it.  The host does not wait: evaluations already
 * enqueued on any stream this ctx has seen read the snapshot as it was, later ones the new one.  With ONE caller stream the
 * two kernels are enqueued on that stream (no event, no cross-stream wait: an [update + bindings-only pick] loop runs 32 us per
 * iteration instead of 49); with several, on the ctx's own stream, ordered by events (KSCHED_OPT_SNAPSHOT_STREAM).
 * If a HIP call fails midway the snapshot is invalidated (KSCHED_E_STATE until the next ksched_set_nodes).
 */
int ksched_update_nodes(ksched_ctx *ctx, uint32_t count, const uint32_t *node_index, const int64_t *avail_cpu_milli,
                        const int64_t *avail_mem_bytes);

/* The node-watch twin of ksched_update_nodes: the labels (and optionally the taints) of `count` nodes changed -- a node was relabelled
 * or tainted (the reference's node reflector, src/main.rs:134-139, makes every such change visible to the next pick:
 * src/predicates.rs:28-31, 49-50).  Host pointers, copied before return; the call does not wait for the device.
 *   node_index    : [count] canonical node indexes (< ksched_num_nodes)
 *   label_val_ids : [n_keys][count] with n_keys = ksched_num_keys: ALL of a listed node's label ids are replaced (column k of the
 *                   update starts count entries after column k - 1's, the [k][n] convention of ksched_set_nodes); NULL when n_keys == 0
 *   taints        : [count] the nodes' new taint bits, or NULL = taints unchanged.  Allowed on a snapshot set without taints: every
 *                   other node then has taint bits 0.
 * `available` is not touched (that is ksched_update_nodes).  A node listed twice takes its last row; count == 0 is a no-op.
 * Afterwards every evaluation entry point gives the same bits as after a ksched_set_nodes with the updated columns.
 * Cost: while every new id is at most its key's largest id when the bitmap index's layout was planned, and every new taint bit falls
 * in its planned taint groups, only the named rows and list-key slots of the touched 1024-node tiles are rebuilt (the index is then
 * bit-identical to a fresh build that plans the same layout: ksched_index_checksum); otherwise the layout is planned again for the
 * union of the old and the new maxima and bits, and the whole index is rebuilt from the columns on the device (a layout outside the
 * fused kernel's limits leaves the snapshot to the direct kernel, as ksched_set_nodes does).  The best-fit ORDER does not change
 * (it reads `available` only): the next KSCHED_PICK_BESTFIT request rebuilds its row bitmaps alone, without sorting.
 * Ordering as ksched_update_nodes (KSCHED_OPT_SNAPSHOT_STREAM): evaluations already enqueued read the old labels, later ones the new.
 * Errors: KSCHED_E_STATE before ksched_set_nodes; KSCHED_E_INVAL, with nothing changed, for an index >= ksched_num_nodes, an id equal
 * to KSCHED_SEL_NEVER, or label_val_ids == NULL while n_keys > 0.  If a HIP call fails midway the snapshot is invalidated
 * (KSCHED_E_STATE until the next ksched_set_nodes).  Added in ABI 7 after its first release: detect it by its symbol. */
int ksched_update_node_labels(ksched_ctx *ctx, uint32_t count, const uint32_t *node_index, const uint32_t *label_val_ids,
                              const uint64_t *taints);

/* Apply a batch's bindings to the snapshot on the device: the step "bind -> shrink `available`" of the scheduler loop
 * evaluate -> bind -> apply -> evaluate, without a host round trip (every successful POST, src/main.rs:94-103, changes what the
 * next LIST of can_pod_fit sees, src/predicates.rs:27-38).  Device pointers, all of them [p]:
 *   bindings      : node index per pod (what ksched_eval_device wrote; -1 = no node)
 *   req_cpu_milli, req_mem_bytes : the pods' requests, as given to the evaluation
 *   ok            : nonzero = the POST landed; NULL = every POST landed
 *   status_out    : per-pod KSCHED_APPLY_* status, or NULL
 * A pod is ELIGIBLE when 0 <= bindings[i] < ksched_num_nodes and (ok == NULL or ok[i] != 0).  For every node the new `available`
 * is old - (sum of req) over the eligible ACCEPTED pods bound to it (old + sum with KSCHED_APPLY_RELEASE), per resource: SubAssign,
 * src/util.rs:31-36.  Without KSCHED_APPLY_FIRST_PER_NODE every eligible pod is accepted; with it, per node only the lowest eligible
 * pod index (one round of the no-over-commit rule of reconcile_batch_sequential); the others are DEFERRED and not applied.
 * The sums are exact and independent of order; when either resource's result leaves int64 NEITHER resource of that node changes
 * and every pod accepted onto it reports KSCHED_APPLY_OVERFLOW.  Same inputs, same bits, on every run.
 * Status precedence: UNBOUND (binding < 0), BAD_NODE (binding >= n), NOT_OK, DEFERRED, then APPLIED or OVERFLOW.
 * Ordering: everything is enqueued behind what `hip_stream` (a hipStream_t; NULL = default stream) already holds -- e.g. the evaluation
 * that wrote `bindings` -- and the host does not wait.  Evaluations already enqueued on any stream this ctx knows read the snapshot as
 * it was, evaluations enqueued afterwards (on any stream) and work enqueued on `hip_stream` afterwards (reading status_out) see the
 * change; the change rides `hip_stream` itself when that is the one caller stream the ctx knows (KSCHED_OPT_SNAPSHOT_STREAM).
 * The input arrays must stay unchanged until that point of `hip_stream`.  The fit part of the bitmap index is rebuilt for the touched
 * 1024-node tiles only; the best-fit order is marked stale (the next KSCHED_PICK_BESTFIT request rebuilds it).
 * Errors: KSCHED_E_STATE before ksched_set_nodes; KSCHED_E_INVAL for NULL required pointers or unknown flags; p == 0 is a no-op.
 * If a HIP call fails midway the snapshot is invalidated (KSCHED_E_STATE until the next ksched_set_nodes). */
#define KSCHED_APPLY_FIRST_PER_NODE 0x01u /* per node accept only the lowest pod index among the eligible pods */
#define KSCHED_APPLY_RELEASE 0x02u        /* add the requests back instead of subtracting (pods deleted / unbound) */
/* KSCHED_APPLY_WHILE_FIT: admit the bindings in pod order while they still fit -- no node is over-committed, and a node takes as many
 * pods of one call as it has room for.  (0x04 and 0x80 are not flags: callers probe with them for KSCHED_E_INVAL.)  An older library of
 * ABI 7 answers KSCHED_E_INVAL to this flag: detect the rule by the constant and that answer; no symbol was added.
 *   Eligibility and the statuses that precede are unchanged: UNBOUND (binding < 0), then BAD_NODE (binding >= n), then NOT_OK.
 *   Per node: the eligible pods bound to it are taken in ascending pod index.  R = (R_cpu, R_mem) starts as the node's `available` at
 *   the call's place in the order of snapshot changes -- so the first pod of a node is checked against the CURRENT value too, which
 *   guards a pipelined caller whose batch i + 1 was evaluated before batch i's apply against stale bindings.
 *     - pod i is admitted iff req_cpu[i] <= R_cpu && req_mem[i] <= R_mem, signed 64-bit compares (can_pod_fit,
 *       src/predicates.rs:37-42): a zero request fits a node at exactly 0 and does not fit a negative one;
 *     - an admitted pod gives R -= req on both resources and reports KSCHED_APPLY_APPLIED;
 *     - a pod that does not fit reports KSCHED_APPLY_DEFERRED and changes nothing; the walk GOES ON behind it (skip, not stop): a
 *       later, smaller pod may still be admitted;
 *     - a pod that fits but whose subtraction would take either resource past INT64_MAX (a negative request only) is not admitted and
 *       reports KSCHED_APPLY_OVERFLOW; the walk goes on -- unlike the summed rule, one such pod does not freeze the node.
 *   The node's new `available` is the final R; a node whose admitted requests sum to zero on both resources is left untouched (its
 *   index tile is not rebuilt for it).  Integer arithmetic in a fixed order: same inputs, same bits, on every run.
 *   KSCHED_APPLY_WHILE_FIT | KSCHED_APPLY_RELEASE and KSCHED_APPLY_WHILE_FIT | KSCHED_APPLY_FIRST_PER_NODE are KSCHED_E_INVAL with
 *   nothing changed; more than 2^31 pods in one call likewise.  Everything else is as without the flag: ordering and
 *   KSCHED_OPT_SNAPSHOT_STREAM, `ok`, `status_out` (may be NULL), p == 0, KSCHED_E_STATE, the invalidation when a HIP call fails after
 *   the change began (the call's scratch is reserved before), the stale best-fit order, the re-index of the touched tiles only.
 *   ksched_apply_bindings_sharded and _sharded_local answer KSCHED_E_UNSUPPORTED to it, with nothing changed, no collective entered
 *   and the clique usable as before: admission needs every rank's requests per node, which the per-node exchange does not carry. */
#define KSCHED_APPLY_WHILE_FIT 0x08u
#define KSCHED_APPLY_APPLIED 0
#define KSCHED_APPLY_UNBOUND 1   /* binding < 0: nothing to apply (no node found) */
#define KSCHED_APPLY_NOT_OK 2    /* ok[p] == 0: the POST did not land (src/main.rs:103-108) */
#define KSCHED_APPLY_DEFERRED 3  /* FIRST_PER_NODE: a lower pod index took this node in this call; WHILE_FIT: the pod did not fit what was left */
#define KSCHED_APPLY_OVERFLOW 4  /* the node's new value would leave int64: node left unchanged (WHILE_FIT: this pod alone is not admitted) */
#define KSCHED_APPLY_BAD_NODE 5  /* binding >= ksched_num_nodes */
int ksched_apply_bindings_device(ksched_ctx *ctx, uint32_t p, const int32_t *bindings, const int64_t *req_cpu_milli,
                                 const int64_t *req_mem_bytes, const uint8_t *ok /* [p] or NULL = all landed */,
                                 uint32_t flags, int32_t *status_out /* [p] or NULL */, void *hip_stream);
/* Host-synchronous read-back of the device's current `available` columns for nodes [first, first + count), ordered behind every
 * snapshot change enqueued so far (set, update, apply).  KSCHED_E_INVAL when the range exceeds ksched_num_nodes. */
int ksched_read_nodes(ksched_ctx *ctx, uint32_t first, uint32_t count, int64_t *out_cpu_milli, int64_t *out_mem_bytes);

/* The ctx remembers every stream a *_device evaluation was enqueued on (that is how snapshot changes are ordered against
 * them without a device-wide wait).  A caller that DESTROYS such a stream while the ctx lives must say so first; streams that
 * outlive the ctx (e.g. a framework's pooled streams) need nothing.  ksched_pipe_destroy does this for the pipe's streams. */
int ksched_forget_stream(ksched_ctx *ctx, void *hip_stream);

/* number of nodes / keys of the current snapshot (0 before ksched_set_nodes) */
uint32_t ksched_num_nodes(const ksched_ctx *ctx);
uint32_t ksched_num_keys(const ksched_ctx *ctx);

/* ---- evaluation, host buffers -------------------------------------------------------------
 * One call = check_node_validity (src/predicates.rs:63-77) for every (pod, node) pair of the
 * batch against the snapshot, plus optionally the pick of select_node_for_pod (src/main.rs:51-71).
 *   req_cpu_milli, req_mem_bytes : [p]   total_pod_resources (src/util.rs:54-75), encoded
 *   sel_val_ids   : [n_keys][p] or NULL (= no pod has a selector)
 *   tolerations   : [p] or NULL (= tolerate nothing)        -- only read with KSCHED_TAINT
 *   samples       : [p][attempts] node indices or NULL       -- only read with KSCHED_PICK_SAMPLED
 *                   an index >= n is treated as an infeasible draw
 *                   (with KSCHED_PICK_UNIFORM: 32-bit draws, of which entry 0 of every row is read;
 *                   with KSCHED_PICK_SPREAD or KSCHED_PICK_PACK: 32-bit draws, all `attempts` of every row are read)
 *   out_feasible  : [p][W] or NULL
 *   out_fit       : [p][W] or NULL; requires KSCHED_WANT_FIT_MASK
 *   out_binding   : [p] or NULL; requires one of the KSCHED_PICK_* flags; -1 = no node
 * Predicates not selected in `flags` are treated as true.
 * The output arrays may be ordinary pageable memory (the copies run at the link's rate into it: 63 MB of mask in 1.2 ms on an MI355X box); keep them from
 * call to call -- a freshly allocated array is first touched BY the copy, which then takes four times as long (bench.py end_to_end.host_arrays_to_mask).
 */
int ksched_eval(ksched_ctx *ctx, uint32_t p, const int64_t *req_cpu_milli, const int64_t *req_mem_bytes,
                const uint32_t *sel_val_ids, const uint64_t *tolerations, const uint32_t *samples,
                uint32_t attempts, uint32_t flags, uint64_t *out_feasible, uint64_t *out_fit,
                int32_t *out_binding);

/* ---- one host thread, several devices: ksched_eval in two halves ---------------------------------
 * north_star: "the pod batch row-shards across the 8 GPUs of one node with an RCCL allgather of the resulting (pod -> node)
 * bindings".  The reference is ONE process (src/main.rs:127-152); a drop-in host therefore drives n devices from one thread: one
 * ksched_ctx per device, the node snapshot replicated to all of them (ksched_set_nodes / ksched_update_nodes on each), the batch's
 * pod rows cut with ksched_shard_bounds, and per batch
 *     for every device r : ksched_eval_begin(ctx[r], rows [lo_r, hi_r) ...)      copies in + evaluation enqueued, NO host wait
 *     ksched_allgather_bindings_local(comms, n, local[], gathered[], count_per_rank, streams[])
 *     ksched_eval_end(ctx[0], gathered[0], n * count_per_rank, host_table)       one copy of the whole table, one host wait
 *     ksched_eval_end(ctx[r], NULL, 0, NULL) for the others                      (their masks, if asked for, have landed)
 * host_table[r * count_per_rank + i] is the binding of pod row lo_r + i (rows past a shard's end are -1).
 * (kube_scheduler_rs_reference_amd/host/sharded.cpp and rust/src/ksched.rs `ShardedEvaluator` are this loop.)
 *
 * ksched_shard_bounds   the one definition of the row split: rank r owns rows [lo, hi) = [r * c, min(p, (r + 1) * c)),
 *                       c = count_per_rank = ceil(p / nranks); the last ranks may own fewer rows, or none.  Pure arithmetic.
 * ksched_eval_begin     ksched_eval without its last two steps (the copy of the bindings to the host, the host wait):
 *                       host pointers as in ksched_eval, for THIS ctx's rows only; `sel_val_ids` may point INTO the whole batch's
 *                       [n_keys][sel_stride] array (sel_val_ids = all + lo, sel_stride = P: column k of the shard starts
 *                       sel_stride entries after column k - 1's; sel_stride = p for a packed array).  Masks, when asked for, are
 *                       copied to out_feasible / out_fit ([p][W], packed) behind the evaluation on the same stream: they are
 *                       complete after ksched_eval_end.  With a pick the bindings stay ON THE DEVICE in a ctx-owned buffer of
 *                       max(p, binding_capacity) int32 -- entries [p, binding_capacity) are -1, the padding the all-gather of
 *                       unequal shards needs -- returned through *binding_dev; *hip_stream is the ctx's own stream, where all of
 *                       this was enqueued (pass both to ksched_allgather_bindings*).  p = 0 is allowed (an empty shard still
 *                       takes part in the exchange).  The input arrays and the two host mask arrays must stay alive and untouched
 *                       until ksched_eval_end has returned (the copies are asynchronous).  The device buffers are valid until the
 *                       next ksched_eval / ksched_eval_begin on the ctx.
 * ksched_gather_buffer  a ctx-owned device buffer of `count` int32 for the gathered table (grown on demand, reused).
 * ksched_eval_end       enqueue the copy of `count` int32 from `bindings_dev` (any device pointer: the gathered table, or
 *                       *binding_dev itself) to `out_host` on the ctx's stream -- skipped when out_host is NULL -- and wait for
 *                       the stream. */
void ksched_shard_bounds(uint32_t p, uint32_t nranks, uint32_t rank, uint32_t *lo, uint32_t *hi, uint32_t *count_per_rank);
int ksched_eval_begin(ksched_ctx *ctx, uint32_t p, const int64_t *req_cpu_milli, const int64_t *req_mem_bytes,
                      const uint32_t *sel_val_ids, uint32_t sel_stride, const uint64_t *tolerations, const uint32_t *samples,
                      uint32_t attempts, uint32_t flags, uint64_t *out_feasible, uint64_t *out_fit, uint32_t binding_capacity,
                      int32_t **binding_dev, void **hip_stream);
int ksched_gather_buffer(ksched_ctx *ctx, uint32_t count, int32_t **dev);
int ksched_eval_end(ksched_ctx *ctx, const int32_t *bindings_dev, uint32_t count, int32_t *out_host);

/* ---- evaluation, device buffers -----------------------------------------------------------
 * Same contract with every array already resident in HBM.  out_feasible may be NULL only when
 * no pick is requested and out_fit is given; when a pick is requested without out_feasible the
 * library uses an internal scratch mask.  `hip_stream` is a hipStream_t (NULL = default stream).
 */
int ksched_eval_device(ksched_ctx *ctx, uint32_t p, const int64_t *req_cpu_milli, const int64_t *req_mem_bytes,
                       const uint32_t *sel_val_ids, const uint64_t *tolerations, const uint32_t *samples,
                       uint32_t attempts, uint32_t flags, uint64_t *out_feasible, uint64_t *out_fit,
                       int32_t *out_binding, void *hip_stream);

/* Same, with the output masks pitched: row `pod` of out_feasible / out_fit starts at word
 * pod * mask_pitch_words (mask_pitch_words >= ksched_mask_words(n)); words [W, pitch) of a row are padding
 * and are written as zero or left untouched.  ksched_mask_pitch(n) rounds W up to a multiple of 16 words
 * (128 bytes), which keeps every row on cache-line boundaries: on MI355X the mask stream then runs at the
 * HBM write ceiling instead of ~70 % of it ("row pitch").  ksched_eval_device == this with
 * mask_pitch_words = W. */
int ksched_eval_device_pitched(ksched_ctx *ctx, uint32_t p, const int64_t *req_cpu_milli, const int64_t *req_mem_bytes,
                               const uint32_t *sel_val_ids, const uint64_t *tolerations, const uint32_t *samples,
                               uint32_t attempts, uint32_t flags, uint64_t *out_feasible, uint64_t *out_fit,
                               int32_t *out_binding, uint32_t mask_pitch_words, void *hip_stream);
uint32_t ksched_mask_pitch(uint32_t n_nodes);

/* ---- mask buffers allocated by the library (ABI 6) ---------------------------------------------
 * The reference never materialises a mask (check_node_validity answers one pair at a time, src/predicates.rs:63-77); the batched
 * path's mask is its own artefact and 92 % of its HBM traffic, and on MI355X the rate at which the mask kernel runs depends on the
 * PHYSICAL placement of the buffer it writes (two rates, 4 % apart at 100k x 5k and 20 % apart at 125k x 50k:
 * profiles/r05_bimodal_by_allocation.md, profiles/r06_mask_alloc.md).  A caller may keep allocating its own masks (any device pointer works);
 * ksched_mask_alloc hands out [p] rows at the pitch ksched_mask_pitch(n) gives, placed the way the measurements found fastest.
 *   how            : KSCHED_MASK_ALLOC_AUTO, or one specific path (for re-measuring the choice: tools/alloc_probe.py)
 *   out_pitch_words: receives the row pitch in 64-bit words (pass it to ksched_eval_device_pitched / ksched_pipe_submit); may be NULL
 * KSCHED_E_STATE before ksched_set_nodes (the pitch follows the node count); a snapshot with a different node count needs new masks.
 * ksched_mask_free waits for the device before it unmaps; ksched_destroy frees what the caller left. */
#define KSCHED_MASK_ALLOC_AUTO 0u
#define KSCHED_MASK_ALLOC_PLAIN 1u      /* hipMalloc */
#define KSCHED_MASK_ALLOC_PROBE 11u     /* probe-and-keep: KSCHED_OPT_MASK_PROBE hipMalloc candidates alive at once; the fused mask kernel is timed into each
                                         * (fit only, zero requests, the current snapshot); the fastest is kept, the others are freed */
/* Measurement paths: implemented in the TEST build of the library only (tests/cpp/hooks/libksched_hip.so = the shipped object code +
 * tests/cpp/test_hooks.cpp); the shipped library answers KSCHED_E_UNSUPPORTED.  tools/alloc_probe.py re-measures the choice with them; none
 * selects the fast placement, and HIP's virtual-memory API showed STALE READS on a mapping's first use right after a contiguous allocation was
 * freed in the same process (profiles/r06_mask_alloc.md section 3): AUTO and PROBE never use them. */
#define KSCHED_MASK_ALLOC_VMM 2u        /* hipMemCreate in one piece at the recommended granularity + hipMemAddressReserve + hipMemMap */
#define KSCHED_MASK_ALLOC_VMM_MIN 4u    /* the same at the minimum granularity */
#define KSCHED_MASK_ALLOC_CONTIGUOUS 5u /* hipExtMallocWithFlags(hipDeviceMallocContiguous): one physical range */
#define KSCHED_MASK_ALLOC_SCATTER_2M 8u  /* physical pieces of 2 MiB created one by one (a quarter more than needed), shuffled, mapped at consecutive addresses */
#define KSCHED_MASK_ALLOC_SCATTER_16M 9u /* the same with pieces of 16 MiB */
#define KSCHED_MASK_ALLOC_LAST 11u      /* (3, 6, 7, 10 -- 1 GiB-aligned VMM, uncached, a memory pool, 64 KiB pieces -- were measured in round 6 and removed) */
/* AUTO = PROBE for masks of at least KSCHED_MASK_PROBE_MIN_BYTES when the snapshot has its bitmap index, PLAIN otherwise: no allocation path selects
 * the fast placement, and below that size a buffer's own rate does not stand out of the run-to-run noise */
#define KSCHED_MASK_PROBE_MIN_BYTES 0x8000000u /* 128 MiB */
int ksched_mask_alloc(ksched_ctx *ctx, uint32_t p, uint32_t how, uint64_t **out_mask, uint32_t *out_pitch_words);
int ksched_mask_free(ksched_ctx *ctx, uint64_t *mask);
/* What the latest probe-and-keep allocation of this ctx measured: microseconds per mask kernel launch into each candidate, in candidate order
 * (the kept one is the smallest).  Returns the number of candidates written (<= cap), 0 when the latest ksched_mask_alloc did not probe. */
int ksched_mask_probe_report(ksched_ctx *ctx, double *out_us, uint32_t cap);

/* The pick alone, from a feasibility mask already on the device (a previous ksched_eval_device* call): lets a caller
 * run the mask kernel of batch i + 1 and the pick of batch i on different HIP streams (the two do not depend on each
 * other; the mask of batch i must stay untouched until its pick has run).
 *   flags        : exactly one of KSCHED_PICK_SAMPLED (select_node_for_pod, src/main.rs:51-71: `samples`, `attempts`),
 *                  KSCHED_PICK_BESTFIT (extension E1), KSCHED_PICK_UNIFORM (extension E3: `samples`, `attempts`),
 *                  KSCHED_PICK_SPREAD (extension E4: `samples`, `attempts`; it reads the snapshot's available columns) and
 *                  KSCHED_PICK_PACK (extension E5: as E4);
 *                  KSCHED_FIT tells the best-fit pick that the mask includes the resource fit (then `req_mem_bytes` [p]
 *                  is read to skip candidates that cannot fit)
 *   feasible     : [p] rows, mask_pitch_words apart, as written by ksched_eval_device_pitched
 * Results are identical to requesting the pick in the ksched_eval_device* call that produced the mask. */
int ksched_pick_device(ksched_ctx *ctx, uint32_t p, const uint64_t *feasible, uint32_t mask_pitch_words,
                       const int64_t *req_mem_bytes, const uint32_t *samples, uint32_t attempts, uint32_t flags,
                       int32_t *out_binding, void *hip_stream);
/* The same from HOST masks (rows packed at ksched_mask_words(n) words): copies in, picks on the ctx's own stream, copies the bindings out and
 * waits.  For hosts that combine masks themselves -- the mirror ANDs the masks of a pod whose selector has more keys than one call takes
 * (KSCHED_MAX_KEYS; the reference has no limit, src/predicates.rs:48-53) and lets the device pick from the result. */
int ksched_pick(ksched_ctx *ctx, uint32_t p, const uint64_t *feasible, const int64_t *req_mem_bytes, const uint32_t *samples,
                uint32_t attempts, uint32_t flags, int32_t *out_binding);

/* ---- pipelined evaluation (throughput form) ------------------------------------------------
 * Consecutive batches do not depend on each other, and within a batch the pick only needs the finished mask.  A
 * ksched_pipe runs them software-pipelined on two internal HIP streams: the mask kernel of batch i + 1 on the
 * "mask" stream while the pick of batch i (and whatever the caller enqueues behind it, e.g. the RCCL all-gather of
 * the bindings) is still running on the "pick" stream.  `depth` slots (1 .. 64); the caller owns the per-slot output buffers
 * (device memory) and passes them to every submit, so the library retains nothing but streams and events.
 *
 *   ksched_pipe_submit(slot, ...)  enqueue one batch into `slot` (round-robin 0 .. depth-1):
 *        mask stream : mask kernel into `mask`
 *        pick stream : pick into `binding`
 *      By default the picks do not read the mask (KSCHED_OPT_PICK_FROM_MASK), so the two streams are not ordered
 *      against each other at all: each is in order by itself.  With a mask-reading pick the pick waits for its mask
 *      kernel and the slot's next mask kernel for that pick (events).
 *      `flags` must contain one KSCHED_PICK_* flag; predicates and pick mean what they mean in ksched_eval_device.
 *      All input arrays are device pointers that must be complete before the call and stay untouched until the
 *      slot's pick has run.  A caller that enqueues its own work on the pick stream behind the pick (reading
 *      `binding`) thereby also delays the slot's next use correctly (the next pick of the slot is ordered after it).
 *   ksched_pipe_wait(slot, stream)  make `hip_stream` wait for the slot's pick; stream == NULL blocks the host.
 *   ksched_pipe_wait_mask(slot, stream)  the same for the slot's MASK (the two streams are not ordered against each other, so
 *        a finished pick says nothing about the mask kernel).  Waits for everything submitted to the mask stream so far; the
 *        event is recorded by this call, so consumers that only read bindings pay nothing for it.
 *   ksched_pipe_stream(which)       the internal hipStream_t: 0 = mask stream, 1 = pick stream, 2 .. = the further streams of the
 *        alternate mode over more than two (NULL until a submit has used them).
 *   ksched_pipe_slot_stream(slot)   the stream that carried the slot's latest pick (alternate mode: its whole evaluation): work
 *        enqueued THERE after the submit -- the all-gather of the slot's bindings -- is ordered behind it by the stream itself,
 *        whatever mode the submit ran in (NULL before the slot's first submit).
 * Results are identical to ksched_eval_device_pitched with the same arguments (tests/test_gpu_parity.py).
 */
typedef struct ksched_pipe ksched_pipe;
int ksched_pipe_create(ksched_ctx *ctx, uint32_t depth, ksched_pipe **out);
void ksched_pipe_destroy(ksched_pipe *pipe);
int ksched_pipe_submit(ksched_pipe *pipe, uint32_t slot, uint32_t p, const int64_t *req_cpu_milli, const int64_t *req_mem_bytes,
                       const uint32_t *sel_val_ids, const uint64_t *tolerations, const uint32_t *samples, uint32_t attempts,
                       uint32_t flags, uint64_t *mask, uint32_t mask_pitch_words, int32_t *binding);
int ksched_pipe_wait(ksched_pipe *pipe, uint32_t slot, void *hip_stream);
int ksched_pipe_wait_mask(ksched_pipe *pipe, uint32_t slot, void *hip_stream);
void *ksched_pipe_stream(ksched_pipe *pipe, int which);
void *ksched_pipe_slot_stream(ksched_pipe *pipe, uint32_t slot);

/* ---- reasons ------------------------------------------------------------------------------
 * Host helper: rebuild check_node_validity's result for one pair from the two masks, in the
 * reference's order (fit first: src/predicates.rs:68-70, then selector: :72-74).
 * feasible_row / fit_row point at the pod's row of each mask.
 */
int ksched_reason(const uint64_t *feasible_row, const uint64_t *fit_row, uint32_t node, uint32_t flags);

/* Per-pair reasons, decided on the device: check_node_validity's result (src/predicates.rs:63-77) for `count` listed
 * (pod, node) pairs of an encoded batch -- what the reference logs at WARN for every rejected candidate
 * (src/main.rs:62).  Order: resources (:68-70), then selector (:72-74), then the taint extension.  Two masks cannot
 * tell a selector failure from a taint failure when both predicates are active (ksched_reason then answers
 * NODE_SELECTOR_MISMATCH); this entry point re-checks the listed pairs from the columns and can.
 *   pod columns as in ksched_eval (host pointers, [p]); pair_pod[i] < p, pair_node[i] < ksched_num_nodes
 *   flags : subset of KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT;  out_reason[i] = KSCHED_REASON_* */
int ksched_explain(ksched_ctx *ctx, uint32_t p, const int64_t *req_cpu_milli, const int64_t *req_mem_bytes,
                   const uint32_t *sel_val_ids, const uint64_t *tolerations, uint32_t count, const uint32_t *pair_pod,
                   const uint32_t *pair_node, uint32_t flags, int32_t *out_reason);

/* ---- why is a pod unschedulable: per-pod node counts by reason, on the device ------------------------
 * The reference ends a pod that found no node with a bare NoNodeFound (src/main.rs:116-118) after ATTEMPTS blind draws, and
 * ksched_explain only decides the listed pairs (the rejected draws of src/main.rs:62).  This entry point makes the statement about
 * the whole cluster ("0/5000 nodes are available: 3120 NotEnoughResources, 1880 NodeSelectorMismatch") without a mask:
 * for pod i, out_counts[i][r] is the number of nodes n < ksched_num_nodes for which check_node_validity (src/predicates.rs:63-77)
 * returns reason r, with the precedence ksched_explain documents: resources first (:68-70), then the selector (:72-74), then the taint
 * extension.  Index r is the KSCHED_REASON_* value, so word 0 (KSCHED_REASON_OK) is the number of feasible nodes.  The four words of a
 * pod always add up to ksched_num_nodes; padding bits never count.  Unlike ksched_reason on two masks it tells selector failures from
 * taint failures when both predicates are selected (it sees the three predicates separately).
 *   flags      : a non-empty subset of KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT; predicates not selected are treated as true
 *   pod columns: as in ksched_eval_device (sel_val_ids == NULL = no pod has a selector, tolerations == NULL = tolerate nothing)
 *   out_counts : [p][KSCHED_SUMMARY_WORDS] uint32, device memory; need not be zeroed.  Same inputs, same bits, on every run.
 * It reads the snapshot like an evaluation: a snapshot change (set, update, apply) enqueued before it is visible, one enqueued after it
 * is not; `hip_stream` (a hipStream_t, NULL = default stream) is remembered like the streams of the *_device evaluations, and the host
 * does not wait.  It works on every snapshot an evaluation works on; KSCHED_OPT_KERNEL selects between the kernel over the per-tile
 * bitmap index and the direct one as it does for evaluations (ksched_last_kernel: "fused" / "direct"; KSCHED_OPT_TIMING brackets the
 * call's kernels for ksched_kernel_time_ms).  Cost: the staging, rank searches and row reads of a mask evaluation, 8 bytes written per
 * (pod, 1024-node tile) into ctx-owned scratch and 16 bytes per pod of output instead of the mask.
 * Errors: KSCHED_E_INVAL for a NULL ctx or required pointer (req_cpu_milli, req_mem_bytes, out_counts with p > 0), a flag bit outside
 * the three predicates, or no predicate at all; KSCHED_E_STATE before ksched_set_nodes; p == 0 is a no-op.
 * ksched_summarize is the host-pointer form: copies in, runs on the ctx's own stream, copies out and waits.
 * Added in ABI 7 without a version change: detect them by symbol. */
#define KSCHED_SUMMARY_WORDS 4u /* per pod: [FEASIBLE, NOT_ENOUGH_RESOURCES, NODE_SELECTOR_MISMATCH, TAINT_NOT_TOLERATED] */
int ksched_summarize_device(ksched_ctx *ctx, uint32_t p, const int64_t *req_cpu_milli, const int64_t *req_mem_bytes,
                            const uint32_t *sel_val_ids, const uint64_t *tolerations, uint32_t flags,
                            uint32_t *out_counts /* [p][KSCHED_SUMMARY_WORDS], device */, void *hip_stream);
int ksched_summarize(ksched_ctx *ctx, uint32_t p, const int64_t *req_cpu_milli, const int64_t *req_mem_bytes,
                     const uint32_t *sel_val_ids, const uint64_t *tolerations, uint32_t flags,
                     uint32_t *out_counts /* [p][KSCHED_SUMMARY_WORDS], host */);

/* ---- multi-GPU: all-gather of the (pod -> node) bindings over RCCL / xGMI --------------------
 * The pod batch row-shards over the GPUs of one node (north_star): rank r evaluates pod rows
 * [r * shard, (r + 1) * shard) with its own ksched_ctx against the replicated node snapshot, and ONE all-gather of the
 * int32 bindings (4 B per pod) gives every rank the whole table.  Masks stay on the GPU that produced them.  The
 * reference has no exchange step at all (one process, src/main.rs:127-152); this replaces nothing, it is what makes
 * the batched path span 8 GPUs.
 *
 * Two ways to build the communicator:
 *   one process per GPU : rank 0 calls ksched_comm_unique_id and hands the 128 bytes to the other ranks out of band
 *                         (env, file, TCP store); every rank calls ksched_comm_create(ctx, id, rank, nranks)
 *                         (ncclCommInitRank on the ctx's device; collective: all ranks must call it).
 *   one process, n GPUs : ksched_comm_create_local(ctxs, n, comms) (ncclCommInitAll): comms[i] belongs to ctxs[i].
 * ksched_allgather_bindings enqueues ncclAllGather(int32) on `hip_stream` and returns without syncing:
 *   gathered[r * count_per_rank + i] = rank r's local[i].  Device pointers; every rank passes the same count (pad the
 *   last shard with -1).  Enqueue it on the stream the pick was launched on and no host sync or event is needed.
 * With one process driving n devices the n calls of one collective must be issued together:
 * ksched_allgather_bindings_local wraps them in ncclGroupStart/End (local[i], gathered[i], hip_streams[i] belong to comms[i]).
 * If any of the n calls (or the group's end) fails, the collective is at best half issued: the library then aborts the whole clique
 * (ncclCommAbort), the handles stay valid only for ksched_comm_destroy, and every later call with them returns KSCHED_E_INVAL --
 * create a new clique.  The streams carry no stuck collective afterwards: ksched_eval_end on them returns.
 * RCCL is loaded on first use (dlopen "librccl.so.1"); a process that never calls these never loads it.
 * Test hook (never in production): with $KSCHED_TEST_HOOKS=1, $KSCHED_RCCL_LIB names the library to load instead
 * (tests/cpp/fake_rccl.cpp: n ranks on one GPU); $KSCHED_RCCL_LIB without the switch makes every ksched_comm_* call fail.
 */
#define KSCHED_COMM_ID_BYTES 128u
typedef struct ksched_comm ksched_comm;
int ksched_comm_unique_id(uint8_t *id /* [KSCHED_COMM_ID_BYTES] */);
int ksched_comm_create(ksched_ctx *ctx, const uint8_t *id, int rank, int nranks, ksched_comm **out);
int ksched_comm_create_local(ksched_ctx *const *ctxs, int n, ksched_comm **out /* [n] */);
void ksched_comm_destroy(ksched_comm *comm);
int ksched_comm_rank(const ksched_comm *comm);
int ksched_comm_size(const ksched_comm *comm);
int ksched_allgather_bindings(ksched_comm *comm, const int32_t *local, int32_t *gathered, uint32_t count_per_rank, void *hip_stream);
int ksched_allgather_bindings_local(ksched_comm *const *comms, int n, const int32_t *const *local, int32_t *const *gathered,
                                    uint32_t count_per_rank, void *const *hip_streams);
/* text of the calling thread's last RCCL failure (empty string if none) */
const char *ksched_comm_last_error(void);

/* Keep the replicated snapshots in step: apply a row-sharded batch's bindings on every rank (ksched_apply_bindings_device over the
 * whole batch, with each rank holding only its own rows).  Added in ABI 7 without a version change: detect them by symbol.
 *   per-process form : every rank of `comm` calls ksched_apply_bindings_sharded with its ctx (comm was created for it)
 *   one-process form : ksched_apply_bindings_sharded_local(ctxs, comms, n, ...): ctxs[i] and comms[i] belong to one device
 *                      (ksched_comm_create_local); the per-rank arguments are arrays [n]; ok, status_out, hip_streams may be NULL
 *                      (and entries of ok / status_out NULL), hip_streams NULL = every rank's default stream.
 * Rank r passes `count` pods, rows [row_lo, row_lo + count) of the batch: bindings, requests, ok and status_out as in
 * ksched_apply_bindings_device, device pointers on its device.  bindings may be the rank's part of ksched_gather_buffer or its
 * ksched_eval_device output; padding entries of -1 are UNBOUND.  Pod i of rank r is global pod row_lo + i (the "lowest pod index"
 * of KSCHED_APPLY_FIRST_PER_NODE); row_lo + count must not exceed 0xFFFFFFFF and the ranks' rows must not overlap.
 * After the call every rank's snapshot -- `available`, node records, bitmap index (ksched_index_checksum) -- is what ONE ctx gets
 * from ksched_apply_bindings_device over the concatenation of all ranks' rows, and rank r's status_out is that call's status of its
 * rows.  Flags, statuses, the exactness and the overflow rule are those of ksched_apply_bindings_device.  Every rank's snapshot must
 * hold the same nodes (the one-process form checks the count).
 * Unlike ksched_apply_bindings_device's p == 0 no-op, a rank with count == 0 STILL JOINS: it takes part in the collectives and applies
 * the other ranks' pods.  Each rank exchanges its per-node claims (FIRST_PER_NODE only, 4 B per node) and its per-node partial sums
 * (32 B per node) with one all-gather each, enqueued on the stream that carries its change.
 * Ordering: that of ksched_apply_bindings_device, per rank (behind what `hip_stream` holds, ahead of what is enqueued after; the host
 * does not wait).
 * Errors: KSCHED_E_INVAL for NULL handles or required pointers, a ctx and comm on different devices, unknown flags, an aborted comm,
 * a clique that is not complete (one-process form: every rank once), snapshots of different node counts (one-process form);
 * KSCHED_E_STATE when a ctx has no snapshot.  A failed collective returns KSCHED_E_RCCL (ksched_comm_last_error): the clique is
 * aborted as in ksched_allgather_bindings_local, and every ctx that entered the call loses its snapshot (KSCHED_E_STATE until its
 * next ksched_set_nodes), since the replicas may no longer agree.  A rank of the per-process form that fails before its collectives
 * leaves its peers waiting in them, as any RCCL rank that drops out does. */
int ksched_apply_bindings_sharded(ksched_ctx *ctx, ksched_comm *comm, uint32_t count, uint32_t row_lo, const int32_t *bindings,
                                  const int64_t *req_cpu_milli, const int64_t *req_mem_bytes, const uint8_t *ok /* [count] or NULL */,
                                  uint32_t flags, int32_t *status_out /* [count] or NULL */, void *hip_stream);
int ksched_apply_bindings_sharded_local(ksched_ctx *const *ctxs, ksched_comm *const *comms, int n, const uint32_t *count,
                                        const uint32_t *row_lo, const int32_t *const *bindings, const int64_t *const *req_cpu_milli,
                                        const int64_t *const *req_mem_bytes, const uint8_t *const *ok /* NULL or [n], entries may be NULL */,
                                        uint32_t flags, int32_t *const *status_out /* NULL or [n] */, void *const *hip_streams);

/* ---- measurement --------------------------------------------------------------------------
 * With KSCHED_OPT_TIMING = 1 every ksched_eval* brackets its mask kernel with hipEvents on the
 * launch stream.  ksched_kernel_time_ms synchronises those events and returns the accumulated
 * kernel milliseconds and launch count since the last reset (both reset by the call).
 */
int ksched_kernel_time_ms(ksched_ctx *ctx, double *total_ms, uint64_t *launches);
/* The same measurement launch by launch: writes the duration (ms) of up to `cap` timed mask kernel launches since the
 * last reset, in launch order, returns how many were written (<0 on error) and resets like ksched_kernel_time_ms. */
int ksched_kernel_time_samples(ksched_ctx *ctx, double *out_ms, uint32_t cap);
/* Diagnostics: copy out the trace of the last fused launch (KSCHED_OPT_TRACE = 1): up to max_blocks records of
 * KSCHED_TRACE_WORDS uint64 (100 MHz timestamps); returns the number of blocks of that launch, <0 on error. */
int ksched_trace_read(ksched_ctx *ctx, uint64_t *out, uint32_t max_blocks);
/* Diagnostics: 64-bit checksums of the per-tile bitmap index as it is on the device right now (out[0]: bitmap rows, out[1]:
 * search trees + cnt tables; both 0 when the snapshot has no index).  Waits for pending snapshot work.  Lets tests show that
 * the device-built index, the host-specified one (KSCHED_OPT_INDEX_BUILD) and an incrementally updated one are the same bits. */
int ksched_index_checksum(ksched_ctx *ctx, uint64_t *out /* [2] */);
/* name of the mask kernel variant the last ksched_eval* used ("direct", "indexed", ...) */
const char *ksched_last_kernel(const ksched_ctx *ctx);
/* how the pick of the last ksched_eval* ran: "fused-tile" / "fused" (it rode in the fused mask launch as tile tests / as waves of
 * the fill, KSCHED_OPT_FUSED_PICK), "select" (its own launch testing the drawn candidates), "bestfit-rows", "from-mask"
 * (KSCHED_OPT_PICK_FROM_MASK / no bitmap index), "uniform" (KSCHED_PICK_UNIFORM), "spread" (KSCHED_PICK_SPREAD), "pack" (KSCHED_PICK_PACK), "none" */
const char *ksched_last_pick(const ksched_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* KSCHED_H */
