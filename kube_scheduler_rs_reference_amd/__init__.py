"""MI355X-native batched pods x nodes predicate evaluator (drop-in for the predicate
filter-and-pick path of acrlabs/kube-scheduler-rs-reference).  See DESIGN.md."""
from . import _lib  # noqa: F401
from ._lib import (FIT, SEL, TAINT, PICK_SAMPLED, PICK_BESTFIT, PICK_UNIFORM, PICK_SPREAD, PICK_PACK, WANT_FIT_MASK, COMBINE_AND, COMBINE_OR,
                   COMBINE_ANDNOT, COMBINE_ANY, COMBINE_SOFT, SELOP_EXISTS, SELOP_GT, SELOP_LT, SELOP_ANY, SELOP_TAGGED, SELTAG_SHIFT, SELTAG_ID_MASK, SELTAG_EQ,
                   SELTAG_NE, SELTAG_EXISTS, SELTAG_ABSENT, SELTAG_GT, SELTAG_LT, SEL_TERMS_SHIFT, SEL_TERMS_MASK, MAX_TERMS, SEL_NEVER, KschedError, sel_terms)  # noqa: F401
from .affinity import node_affinity_rows  # noqa: F401
from .evaluator import Evaluator, EvalResult, mask_words, pack_mask, seltag, unpack_mask  # noqa: F401
