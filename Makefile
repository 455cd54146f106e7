# Build of the MI355X-native predicate evaluator.  Everything is built in-tree (the .so files
# travel to the GPU box with the gpurun snapshot; they are git-ignored).
#
#   make            -> lib (HIP C-ABI library) + host (C++ host mirror) + oracle (test-only CPU restatement)
#   make lib        -> kube_scheduler_rs_reference_amd/libksched_hip.so     hipcc, gfx950 only
#   make host       -> kube_scheduler_rs_reference_amd/libksched_host.so    g++, links libksched_hip.so; + tests/cpp/host_tests
#   make oracle     -> oracle/liboracle.so                                  gcc, test infrastructure only
#   make tools      -> tools/pmc_calib                                      hipcc: calibration kernels for the HBM counters
#                      tools/libmask_combine_bench.so                       hipcc: k_mask_combine and k_mask_combine_soft alone, for tools/mask_combine_cost.py
#                                                                           and tools/mask_combine_soft_cost.py
#   make sanitize   -> build/san/host_tests_{asan,tsan}                     the host mirror + its C++ tests under AddressSanitizer + UBSan, and under ThreadSanitizer
#                      (CPU sanitizers over HOST code only; `tools/sanitize.sh` runs them: the CPU half here, the device half on a GPU box)
#   make test-lib   -> tests/cpp/hooks/libksched_hip.so                     the SAME object code + tests/cpp/test_hooks.cpp: the only build in which
#                      $KSCHED_TEST_HOOKS=1 switches on the RCCL stand-in, fault injection and the k-replica shard (the shipped library has none of it)
HIPCC   ?= /opt/rocm/bin/hipcc
CXX     ?= g++
CC      ?= gcc
ARCH    ?= gfx950
PKG     := kube_scheduler_rs_reference_amd
CSRC    := $(PKG)/csrc
HOST    := $(PKG)/host

HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-pass-failed
CXXFLAGS := -O2 -std=c++17 -fPIC -Wall -Wextra -Iinclude
CFLAGS   := -O2 -std=c11 -fPIC -Wall -Wextra -fopenmp

LIB_HIP  := $(PKG)/libksched_hip.so
LIB_HOST := $(PKG)/libksched_host.so
LIB_ORA  := oracle/liboracle.so

HOST_SRCS := $(wildcard $(HOST)/*.cpp)
HOST_HDRS := $(wildcard $(HOST)/*.hpp) include/ksched.h
HOST_TEST := tests/cpp/host_tests
OBJ_TOOL := tests/cpp/objects_eval
FAKE_RCCL := tests/cpp/libfake_rccl.so
INDEX_TEST := tests/cpp/index_tests
PLAN_TEST := tests/cpp/plan_tests
LAUNCH_TEST := tests/cpp/tile_launch_tests
CHANGE_TEST := tests/cpp/snapshot_change_tests
NODE_EVENTS_TEST := tests/cpp/node_events_tests
SUMMARY_TEST := tests/cpp/summary_tests
RANKED_PLAN_TEST := tests/cpp/ranked_plan_tests
UNIFORM_PICK_TEST := tests/cpp/uniform_pick_tests
SPREAD_PICK_TEST := tests/cpp/spread_pick_tests
PACK_PICK_TEST := tests/cpp/pack_pick_tests
BESTFIT_LAYOUT_TEST := tests/cpp/bestfit_layout_tests
PIPE_PLAN_TEST := tests/cpp/pipe_plan_tests
APPLY_ADMIT_TEST := tests/cpp/apply_admit_tests
STREAM_ORDER_TEST := tests/cpp/stream_order_tests
MERGE_SORT_PLAN_TEST := tests/cpp/merge_sort_plan_tests
APPLY_PLAN_TEST := tests/cpp/apply_plan_tests
COMBINE_PLAN_TEST := tests/cpp/combine_plan_tests
SOFT_PLAN_TEST := tests/cpp/soft_plan_tests
SELOP_PLAN_TEST := tests/cpp/selop_plan_tests
SELTAG_PLAN_TEST := tests/cpp/seltag_plan_tests
SELTERMS_PLAN_TEST := tests/cpp/selterms_plan_tests

PMC_CALIB := tools/pmc_calib
COMBINE_BENCH := tools/libmask_combine_bench.so

LIB_OBJ  := $(CSRC)/ksched_api.o
LIB_HIP_TEST := tests/cpp/hooks/libksched_hip.so

.PHONY: all lib host oracle tools clean test-lib sanitize
all: lib test-lib host oracle tools

# kernels of KNOWN byte counts for calibrating the HBM counters (bench.py --live-traffic, tools/gpu_round.sh pmc)
tools: $(PMC_CALIB) $(COMBINE_BENCH)
$(PMC_CALIB): tools/pmc_calib.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ tools/pmc_calib.hip

# k_mask_combine alone, its yardstick (a device-to-device copy) and k_mask_combine_soft alone as three C functions, for
# tools/mask_combine_cost.py and tools/mask_combine_soft_cost.py: the library's own launch paths, compiled from the same headers with the same flags
$(COMBINE_BENCH): tools/mask_combine_bench.hip $(CSRC)/kernels_combine.hpp $(CSRC)/mask_combine.hpp $(CSRC)/kernels_combine_soft.hpp $(CSRC)/mask_combine_soft.hpp include/ksched.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ tools/mask_combine_bench.hip

lib: $(LIB_HIP)
# the kernels are compiled ONCE; the shipped library and the test build are two links of the same object
$(LIB_OBJ): $(CSRC)/ksched_api.hip $(wildcard $(CSRC)/*.hpp) include/ksched.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $(CSRC)/ksched_api.hip
$(LIB_HIP): $(LIB_OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $(LIB_OBJ)
test-lib: $(LIB_HIP_TEST)
$(LIB_HIP_TEST): $(LIB_OBJ) tests/cpp/test_hooks.cpp
	mkdir -p tests/cpp/hooks
	$(CXX) -O2 -std=c++17 -fPIC -Wall -Wextra -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c -o tests/cpp/hooks/test_hooks.o tests/cpp/test_hooks.cpp
	$(HIPCC) --offload-arch=$(ARCH) -shared -Wl,-soname,libksched_hip.so -o $@ $(LIB_OBJ) tests/cpp/hooks/test_hooks.o

# (the plain-g++ tests of csrc/ headers are built where their source is present: a tree that carries an older tests/ still builds everything else)
host: $(LIB_HOST) $(HOST_TEST) $(NODE_EVENTS_TEST) $(SUMMARY_TEST) $(foreach t,$(INDEX_TEST) $(PLAN_TEST) $(LAUNCH_TEST) $(CHANGE_TEST) $(RANKED_PLAN_TEST) $(UNIFORM_PICK_TEST) $(SPREAD_PICK_TEST) $(PACK_PICK_TEST) $(BESTFIT_LAYOUT_TEST) $(PIPE_PLAN_TEST) $(APPLY_ADMIT_TEST) $(STREAM_ORDER_TEST) $(MERGE_SORT_PLAN_TEST) $(APPLY_PLAN_TEST) $(COMBINE_PLAN_TEST) $(SOFT_PLAN_TEST) $(SELOP_PLAN_TEST) $(SELTAG_PLAN_TEST) $(SELTERMS_PLAN_TEST),$(if $(wildcard $(t).cpp),$(t))) $(OBJ_TOOL) $(FAKE_RCCL) $(LIB_HIP_TEST)
# TEST-ONLY stand-in for librccl (n ranks on one GPU; loaded only with KSCHED_TEST_HOOKS=1 + KSCHED_RCCL_LIB, see csrc/comm_rccl.hpp)
$(FAKE_RCCL): tests/cpp/fake_rccl.cpp
	$(CXX) -O2 -std=c++17 -fPIC -Wall -Wextra -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -shared -o $@ tests/cpp/fake_rccl.cpp -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -lrt -lpthread
# host-only check of the bitmap index arithmetic (no GPU, no HIP runtime call): tests/test_index_host.py runs it
$(INDEX_TEST): tests/cpp/index_tests.cpp $(CSRC)/tile_index.hpp
	$(CXX) -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -o $@ tests/cpp/index_tests.cpp
# host-only check of the evaluation plan (csrc/eval_plan.hpp: which kernels a request runs; no GPU, no HIP header): tests/test_eval_plan_host.py runs it
$(PLAN_TEST): tests/cpp/plan_tests.cpp $(CSRC)/eval_plan.hpp $(CSRC)/sel_ops.hpp $(CSRC)/sel_tags.hpp $(CSRC)/sel_terms.hpp $(CSRC)/mask_combine.hpp $(CSRC)/bestfit_layout.hpp $(CSRC)/merge_sort_plan.hpp include/ksched.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/plan_tests.cpp
# host-only check of a tile-kernel launch's description (csrc/tile_launch.hpp: LDS carve-up, launch geometry, argument fill, predicate dispatch; no GPU, no HIP runtime call): tests/test_tile_launch_host.py runs it
$(LAUNCH_TEST): tests/cpp/tile_launch_tests.cpp $(CSRC)/tile_launch.hpp $(CSRC)/tile_index.hpp $(CSRC)/eval_request.hpp include/ksched.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -Wno-attributes -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -o $@ tests/cpp/tile_launch_tests.cpp
# host-only check of the pure parts of a snapshot change (csrc/snapshot_change.hpp: kept rows, layout decision, staging offsets, what is stale; no GPU, no HIP header): tests/test_snapshot_change_host.py runs it
$(CHANGE_TEST): tests/cpp/snapshot_change_tests.cpp $(CSRC)/snapshot_change.hpp include/ksched.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/snapshot_change_tests.cpp
# host-only check of the plan of a ranked-pick request, KSCHED_PICK_UNIFORM / _SPREAD / _PACK (csrc/eval_plan.hpp, csrc/pipe_plan.hpp; no GPU, no HIP header): tests/test_ranked_plan_host.py runs it
$(RANKED_PLAN_TEST): tests/cpp/ranked_plan_tests.cpp $(CSRC)/eval_plan.hpp $(CSRC)/sel_ops.hpp $(CSRC)/sel_tags.hpp $(CSRC)/sel_terms.hpp $(CSRC)/mask_combine.hpp $(CSRC)/pipe_plan.hpp $(CSRC)/bestfit_layout.hpp $(CSRC)/merge_sort_plan.hpp include/ksched.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/ranked_plan_tests.cpp
# host-only check of the numbers the best-fit structures and launches are sized by (csrc/bestfit_layout.hpp: order, row and hand-over layouts, counter rotation, debug bits; no GPU, no HIP header): tests/test_bestfit_layout_host.py runs it
$(BESTFIT_LAYOUT_TEST): tests/cpp/bestfit_layout_tests.cpp $(CSRC)/bestfit_layout.hpp $(CSRC)/merge_sort_plan.hpp
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/bestfit_layout_tests.cpp
# host-only check of a pipe submit's plan (csrc/pipe_plan.hpp: streams, event waits, the slot's next state, over a happens-before model of every sequence of four submits; no GPU, no HIP header): tests/test_pipe_plan_host.py runs it
$(PIPE_PLAN_TEST): tests/cpp/pipe_plan_tests.cpp $(CSRC)/pipe_plan.hpp include/ksched.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/pipe_plan_tests.cpp
# host-only check of KSCHED_APPLY_WHILE_FIT's chunk walk (csrc/apply_admit.hpp: a 64-lane emulation of k_apply_admit against the serial rule; no GPU, no HIP header): tests/test_admit_host.py runs it
$(APPLY_ADMIT_TEST): tests/cpp/apply_admit_tests.cpp $(CSRC)/apply_admit.hpp
	$(CXX) -O2 -std=c++17 -Wall -Wextra -pthread -o $@ tests/cpp/apply_admit_tests.cpp
# host-only check of the ctx's stream ordering (csrc/stream_order.hpp: every stream wait, over a happens-before model of every sequence of up to five calls, against the rules as they were, and the steady states call by call; no GPU, no HIP header): tests/test_stream_order_host.py runs it
$(STREAM_ORDER_TEST): tests/cpp/stream_order_tests.cpp $(CSRC)/stream_order.hpp
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/stream_order_tests.cpp
# host-only check of the device merge sort's plan (csrc/merge_sort_plan.hpp: passes, grids and buffers of every step, executed on the CPU with the stale set poisoned, and step by step against the two drivers as they were; no GPU, no HIP header): tests/test_merge_sort_plan_host.py runs it
$(MERGE_SORT_PLAN_TEST): tests/cpp/merge_sort_plan_tests.cpp $(CSRC)/merge_sort_plan.hpp
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/merge_sort_plan_tests.cpp
# host-only check of an apply call's plan (csrc/apply_plan.hpp: flag verdict, scratch step, passes and grids per rank, collectives, against the five functions as they were; no GPU, no HIP header): tests/test_apply_plan_host.py runs it
$(APPLY_PLAN_TEST): tests/cpp/apply_plan_tests.cpp $(CSRC)/apply_plan.hpp $(CSRC)/merge_sort_plan.hpp include/ksched.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/apply_plan_tests.cpp
# host-only check of a combining evaluation's rules (csrc/mask_combine.hpp: the op of a flag word, the argument rules, the valid-bits word, the access width, the launch geometry executed on the CPU; csrc/eval_plan.hpp: the plan with an op, and without one against plan_eval as it was; no GPU, no HIP header): tests/test_combine_plan_host.py runs it
$(COMBINE_PLAN_TEST): tests/cpp/combine_plan_tests.cpp $(CSRC)/mask_combine.hpp $(CSRC)/eval_plan.hpp $(CSRC)/sel_ops.hpp $(CSRC)/sel_tags.hpp $(CSRC)/sel_terms.hpp $(CSRC)/bestfit_layout.hpp $(CSRC)/merge_sort_plan.hpp include/ksched.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/combine_plan_tests.cpp
# host-only check of a soft combining evaluation's rules, KSCHED_COMBINE_SOFT (csrc/mask_combine_soft.hpp: which flag words and entry points carry the modifier, the row rule, the launch geometry executed on the CPU at each side of every switch; csrc/eval_plan.hpp: the plan with the bit against the plain combining plan; no GPU, no HIP header): tests/test_soft_plan_host.py runs it
$(SOFT_PLAN_TEST): tests/cpp/soft_plan_tests.cpp $(CSRC)/mask_combine_soft.hpp $(CSRC)/mask_combine.hpp $(CSRC)/eval_plan.hpp $(CSRC)/sel_ops.hpp $(CSRC)/sel_tags.hpp $(CSRC)/sel_terms.hpp $(CSRC)/bestfit_layout.hpp $(CSRC)/merge_sort_plan.hpp include/ksched.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/soft_plan_tests.cpp
# host-only check of an operator call's rules, KSCHED_SELOP_EXISTS / _GT / _LT (csrc/sel_ops.hpp: the operator of a flag word, the argument rules, the rule for one pair and one row, the launch geometry walked on the CPU; csrc/eval_plan.hpp: the plan of an operator call, and without an operator against plan_eval as it was; no GPU, no HIP header): tests/test_selop_plan_host.py runs it
$(SELOP_PLAN_TEST): tests/cpp/selop_plan_tests.cpp $(CSRC)/sel_ops.hpp $(CSRC)/sel_tags.hpp $(CSRC)/sel_terms.hpp $(CSRC)/mask_combine_soft.hpp $(CSRC)/mask_combine.hpp $(CSRC)/eval_plan.hpp $(CSRC)/bestfit_layout.hpp $(CSRC)/merge_sort_plan.hpp include/ksched.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/selop_plan_tests.cpp
# host-only check of a tagged call's rules, KSCHED_SELOP_TAGGED (csrc/sel_tags.hpp: the argument rules, the entry's tag and id, the rule for one pair and one row, the one compare form the kernel decodes every tag into, the launch geometry walked on the CPU; csrc/eval_plan.hpp: the plan of a tagged call, and without the flag against plan_eval as it was; no GPU, no HIP header): tests/test_seltag_plan_host.py runs it
$(SELTAG_PLAN_TEST): tests/cpp/seltag_plan_tests.cpp $(CSRC)/sel_tags.hpp $(CSRC)/sel_terms.hpp $(CSRC)/sel_ops.hpp $(CSRC)/mask_combine_soft.hpp $(CSRC)/mask_combine.hpp $(CSRC)/eval_plan.hpp $(CSRC)/bestfit_layout.hpp $(CSRC)/merge_sort_plan.hpp include/ksched.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/seltag_plan_tests.cpp
# host-only check of a tagged call's term count, KSCHED_SEL_TERMS (csrc/sel_terms.hpp: the count of a flag word, the argument rules, where an entry lies, one pod's row against seltag_row, the launch geometry walked on the CPU for both kernels; csrc/eval_plan.hpp: the plan with the field, and without it against plan_eval as it was; no GPU, no HIP header): tests/test_selterms_plan_host.py runs it
$(SELTERMS_PLAN_TEST): tests/cpp/selterms_plan_tests.cpp $(CSRC)/sel_terms.hpp $(CSRC)/sel_tags.hpp $(CSRC)/sel_ops.hpp $(CSRC)/mask_combine_soft.hpp $(CSRC)/mask_combine.hpp $(CSRC)/eval_plan.hpp $(CSRC)/bestfit_layout.hpp $(CSRC)/merge_sort_plan.hpp include/ksched.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/selterms_plan_tests.cpp
$(LIB_HOST): $(HOST_SRCS) $(HOST_HDRS) $(LIB_HIP)
	$(CXX) $(CXXFLAGS) -shared -o $@ $(HOST_SRCS) -L$(PKG) -lksched_hip -Wl,-rpath,'$$ORIGIN' -lpthread
# C++ tests of the host mirror (tests/cpp/host_tests.cpp; driven by tests/test_host_mirror.py)
$(HOST_TEST): tests/cpp/host_tests.cpp $(LIB_HOST) $(HOST_HDRS)
	$(CXX) $(CXXFLAGS) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ tests/cpp/host_tests.cpp -L$(PKG) -lksched_host -lksched_hip -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../$(PKG)' -Wl,-rpath,/opt/rocm/lib -lpthread -ldl

# C++ tests of Snapshot::observe_nodes / Context::observe_nodes (tests/cpp/node_events_tests.cpp; driven by tests/test_node_events.py)
$(NODE_EVENTS_TEST): tests/cpp/node_events_tests.cpp $(LIB_HOST) $(HOST_HDRS)
	$(CXX) $(CXXFLAGS) -o $@ tests/cpp/node_events_tests.cpp -L$(PKG) -lksched_host -lksched_hip -Wl,-rpath,'$$ORIGIN/../../$(PKG)' -lpthread

# C++ tests of explain_unschedulable / format_unschedulable / Context::explain_no_node_found (tests/cpp/summary_tests.cpp; driven by tests/test_summary_host.py)
$(SUMMARY_TEST): tests/cpp/summary_tests.cpp tests/cpp/json_min.hpp $(LIB_HOST) $(HOST_HDRS)
	$(CXX) $(CXXFLAGS) -o $@ tests/cpp/summary_tests.cpp -L$(PKG) -lksched_host -lksched_hip -Wl,-rpath,'$$ORIGIN/../../$(PKG)' -lpthread

# C++ tests of Context::pick_uniform (tests/cpp/uniform_pick_tests.cpp; driven by tests/test_uniform_host.py)
$(UNIFORM_PICK_TEST): tests/cpp/uniform_pick_tests.cpp tests/cpp/json_min.hpp $(LIB_HOST) $(HOST_HDRS) $(FAKE_RCCL) $(LIB_HIP_TEST)
	$(CXX) $(CXXFLAGS) -o $@ tests/cpp/uniform_pick_tests.cpp -L$(PKG) -lksched_host -lksched_hip -Wl,-rpath,'$$ORIGIN/../../$(PKG)' -lpthread

# C++ tests of Context::pick_spread (tests/cpp/spread_pick_tests.cpp; driven by tests/test_spread_host.py)
$(SPREAD_PICK_TEST): tests/cpp/spread_pick_tests.cpp tests/cpp/json_min.hpp tests/cpp/objects_json.hpp $(LIB_HOST) $(HOST_HDRS) $(FAKE_RCCL) $(LIB_HIP_TEST)
	$(CXX) $(CXXFLAGS) -o $@ tests/cpp/spread_pick_tests.cpp -L$(PKG) -lksched_host -lksched_hip -Wl,-rpath,'$$ORIGIN/../../$(PKG)' -lpthread

# C++ tests of Context::pick_pack (tests/cpp/pack_pick_tests.cpp; driven by tests/test_gpu_pack_host.py)
$(PACK_PICK_TEST): tests/cpp/pack_pick_tests.cpp tests/cpp/json_min.hpp tests/cpp/objects_json.hpp $(LIB_HOST) $(HOST_HDRS) $(FAKE_RCCL) $(LIB_HIP_TEST)
	$(CXX) $(CXXFLAGS) -o $@ tests/cpp/pack_pick_tests.cpp -L$(PKG) -lksched_host -lksched_hip -Wl,-rpath,'$$ORIGIN/../../$(PKG)' -lpthread

# objects JSON -> host encoder -> device, printed for the Python parity tests (tests/test_gpu_objects.py)
$(OBJ_TOOL): tests/cpp/objects_eval.cpp tests/cpp/json_min.hpp $(LIB_HOST) $(HOST_HDRS)
	$(CXX) $(CXXFLAGS) -o $@ tests/cpp/objects_eval.cpp -L$(PKG) -lksched_host -lksched_hip -Wl,-rpath,'$$ORIGIN/../../$(PKG)' -lpthread

# Host-side sanitizer builds (g++; the evaluator library they link is the ordinary test build: device code is not instrumented)
SAN_DIR  := build/san
SAN_SRCS := tests/cpp/host_tests.cpp $(HOST_SRCS)
SAN_FLAGS := -O1 -g -std=c++17 -fPIC -Wall -Wextra -Iinclude -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -fno-omit-frame-pointer
SAN_LINK := -Ltests/cpp/hooks -lksched_hip -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../tests/cpp/hooks' -Wl,-rpath,/opt/rocm/lib -lpthread -ldl
SAN_OBJ_SRCS := tests/cpp/objects_eval.cpp $(HOST_SRCS)
SAN_NODE_SRCS := tests/cpp/node_events_tests.cpp $(HOST_SRCS)
sanitize: $(SAN_DIR)/host_tests_asan $(SAN_DIR)/host_tests_tsan $(SAN_DIR)/objects_eval_asan $(SAN_DIR)/objects_eval_tsan $(SAN_DIR)/node_events_tests_asan
$(SAN_DIR)/asan/%.o: %.cpp $(HOST_HDRS)
	mkdir -p $(dir $@)
	$(CXX) $(SAN_FLAGS) -fsanitize=address,undefined -c -o $@ $<
$(SAN_DIR)/tsan/%.o: %.cpp $(HOST_HDRS)
	mkdir -p $(dir $@)
	$(CXX) $(SAN_FLAGS) -fsanitize=thread -c -o $@ $<
$(SAN_DIR)/asan/tests/cpp/objects_eval.o $(SAN_DIR)/tsan/tests/cpp/objects_eval.o: tests/cpp/json_min.hpp
# the objects -> reconcile_batch -> POST sink -> snapshot loop at any size (tools/host_loop.py with OBJECTS_EVAL_BIN): the threaded path at production batch sizes
$(SAN_DIR)/objects_eval_asan: $(SAN_OBJ_SRCS:%.cpp=$(SAN_DIR)/asan/%.o) $(LIB_HIP_TEST)
	$(CXX) -fsanitize=address,undefined -o $@ $(SAN_OBJ_SRCS:%.cpp=$(SAN_DIR)/asan/%.o) $(SAN_LINK)
$(SAN_DIR)/objects_eval_tsan: $(SAN_OBJ_SRCS:%.cpp=$(SAN_DIR)/tsan/%.o) $(LIB_HIP_TEST)
	$(CXX) -fsanitize=thread -o $@ $(SAN_OBJ_SRCS:%.cpp=$(SAN_DIR)/tsan/%.o) $(SAN_LINK)
# the node-event sequences and the seeded walk (node_events_tests cpu / walk: encode-only, no device call) under AddressSanitizer + UBSan
$(SAN_DIR)/node_events_tests_asan: $(SAN_NODE_SRCS:%.cpp=$(SAN_DIR)/asan/%.o) $(LIB_HIP_TEST)
	$(CXX) -fsanitize=address,undefined -o $@ $(SAN_NODE_SRCS:%.cpp=$(SAN_DIR)/asan/%.o) $(SAN_LINK)
$(SAN_DIR)/host_tests_asan: $(SAN_SRCS:%.cpp=$(SAN_DIR)/asan/%.o) $(LIB_HIP_TEST)
	$(CXX) -fsanitize=address,undefined -o $@ $(SAN_SRCS:%.cpp=$(SAN_DIR)/asan/%.o) $(SAN_LINK)
$(SAN_DIR)/host_tests_tsan: $(SAN_SRCS:%.cpp=$(SAN_DIR)/tsan/%.o) $(LIB_HIP_TEST)
	$(CXX) -fsanitize=thread -o $@ $(SAN_SRCS:%.cpp=$(SAN_DIR)/tsan/%.o) $(SAN_LINK)

oracle: $(LIB_ORA)
$(LIB_ORA): oracle/oracle.c oracle/oracle.h
	$(CC) $(CFLAGS) -shared -o $@ oracle/oracle.c

clean:
	rm -f $(LIB_OBJ) $(LIB_HIP_TEST) tests/cpp/hooks/test_hooks.o $(LIB_HIP) $(LIB_HOST) $(LIB_ORA) $(HOST_TEST) $(NODE_EVENTS_TEST) $(SUMMARY_TEST) $(INDEX_TEST) $(PLAN_TEST) $(LAUNCH_TEST) $(CHANGE_TEST) $(RANKED_PLAN_TEST) $(UNIFORM_PICK_TEST) $(SPREAD_PICK_TEST) $(PACK_PICK_TEST) $(BESTFIT_LAYOUT_TEST) $(PIPE_PLAN_TEST) $(APPLY_ADMIT_TEST) $(STREAM_ORDER_TEST) $(MERGE_SORT_PLAN_TEST) $(APPLY_PLAN_TEST) $(COMBINE_PLAN_TEST) $(SOFT_PLAN_TEST) $(SELOP_PLAN_TEST) $(SELTAG_PLAN_TEST) $(SELTERMS_PLAN_TEST) $(OBJ_TOOL) $(FAKE_RCCL) $(PMC_CALIB) $(COMBINE_BENCH)
