# Top-level build of the MI355X (gfx950) SVGD library and test/bench helpers.
#   make            -> svgdcpp_amd/libsvgdcpp_amd.so (HIP kernels + C ABI, links RCCL)
#   make oracle     -> oracle/liboracle.so (CPU restatement; test infrastructure)
#   make cpp        -> build/{mvn_example,gmm_example,svgd_run_bench,test_api,test_dist,test_ksd,test_glm,test_glm_hess,test_glm_predict,test_imq,test_ksd_imq,test_thin,test_mmd} (SVGDCpp-compatible C++ API)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-result
SRC_DIR := svgdcpp_amd/csrc
LIB := svgdcpp_amd/libsvgdcpp_amd.so
# the runtime behind the C ABI: svgd_capi.cpp and one unit per phase (ctx.h)
CTX_OBJS := $(SRC_DIR)/svgd_capi.o $(SRC_DIR)/ctx_comm.o $(SRC_DIR)/ctx_timing.o $(SRC_DIR)/ctx_median.o $(SRC_DIR)/ctx_phi.o \
        $(SRC_DIR)/ctx_create.o $(SRC_DIR)/ctx_host_step.o $(SRC_DIR)/ctx_models.o $(SRC_DIR)/ctx_ksd.o $(SRC_DIR)/ctx_predict.o $(SRC_DIR)/ctx_thin.o \
        $(SRC_DIR)/ctx_mmd.o
OBJS := $(SRC_DIR)/svgd_kernels.o $(SRC_DIR)/svgd_collect.o $(SRC_DIR)/svgd_ksd.o $(CTX_OBJS) $(SRC_DIR)/plan.o $(SRC_DIR)/median_plan.o $(SRC_DIR)/host_models.o \
        $(SRC_DIR)/hostcomm.o $(SRC_DIR)/svgd_glm.o $(SRC_DIR)/svgd_glm_predict.o $(SRC_DIR)/svgd_gauss_hess.o $(SRC_DIR)/host_glm.o \
        $(SRC_DIR)/svgd_imq.o $(SRC_DIR)/host_imq.o $(SRC_DIR)/svgd_ksd_imq.o $(SRC_DIR)/host_ksd.o \
        $(SRC_DIR)/svgd_thin.o $(SRC_DIR)/host_thin.o $(SRC_DIR)/svgd_mmd.o $(SRC_DIR)/host_mmd.o
HDRS := $(SRC_DIR)/svgd_kernels.h $(SRC_DIR)/select_state.h $(SRC_DIR)/median_plan.h $(SRC_DIR)/built.h $(SRC_DIR)/dispatch.h $(SRC_DIR)/plan.h $(SRC_DIR)/svgd_ksd.h $(SRC_DIR)/svgd_device.h $(SRC_DIR)/svgd_exp_table.h \
        $(SRC_DIR)/svgd_glm.h $(SRC_DIR)/svgd_glm_dev.h $(SRC_DIR)/svgd_glm_predict.h $(SRC_DIR)/svgd_gauss_hess.h $(SRC_DIR)/host_glm.h include/svgdcpp_amd/svgd_capi.h \
        $(SRC_DIR)/ctx.h $(SRC_DIR)/resource.h $(SRC_DIR)/hostcomm.h $(SRC_DIR)/host_models.h $(SRC_DIR)/svgd_imq.h \
        $(SRC_DIR)/svgd_imq_dev.h $(SRC_DIR)/svgd_ksd_imq.h $(SRC_DIR)/svgd_thin.h $(SRC_DIR)/svgd_mmd.h

all: $(LIB)

$(SRC_DIR)/%.o: $(SRC_DIR)/%.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the matrix-core collect pass keeps its MFMA accumulators in VGPRs (gfx950's
# unified register file): no AGPR copies in its classification loop
$(SRC_DIR)/svgd_collect.o: $(SRC_DIR)/svgd_collect.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -mllvm -amdgpu-mfma-vgpr-form -c $< -o $@

$(CTX_OBJS): $(SRC_DIR)/%.o: $(SRC_DIR)/%.cpp $(HDRS)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

# the link's object list, for the variant builds (tools/build_*_variant*.sh)
print-objs:
	@echo $(OBJS)

# host-only translation units (no device code)
$(SRC_DIR)/plan.o: $(SRC_DIR)/plan.cpp $(HDRS)
	$(CXX) -O3 -std=c++17 -fPIC -Wall -c $< -o $@

$(SRC_DIR)/median_plan.o: $(SRC_DIR)/median_plan.cpp $(HDRS)
	$(CXX) -O3 -std=c++17 -fPIC -Wall -c $< -o $@

$(SRC_DIR)/hostcomm.o: $(SRC_DIR)/hostcomm.cpp $(SRC_DIR)/hostcomm.h
	$(HIPCC) -O2 -std=c++17 -fPIC -Wall -c $< -o $@

$(SRC_DIR)/host_models.o: $(SRC_DIR)/host_models.cpp $(SRC_DIR)/host_grad_block.inc $(SRC_DIR)/host_grad_soa8.inc $(HDRS)
	$(CXX) -O3 -std=c++17 -fPIC -fopenmp -Wall -Wno-psabi -c $< -o $@

$(SRC_DIR)/host_glm.o: $(SRC_DIR)/host_glm.cpp $(HDRS)
	$(CXX) -O3 -std=c++17 -fPIC -fopenmp -Wall -c $< -o $@

$(SRC_DIR)/host_imq.o: $(SRC_DIR)/host_imq.cpp $(HDRS)
	$(CXX) -O3 -std=c++17 -fPIC -fopenmp -Wall -c $< -o $@

$(SRC_DIR)/host_ksd.o: $(SRC_DIR)/host_ksd.cpp $(HDRS)
	$(CXX) -O3 -std=c++17 -fPIC -fopenmp -Wall -c $< -o $@

$(SRC_DIR)/host_thin.o: $(SRC_DIR)/host_thin.cpp $(HDRS)
	$(CXX) -O3 -std=c++17 -fPIC -fopenmp -Wall -c $< -o $@

$(SRC_DIR)/host_mmd.o: $(SRC_DIR)/host_mmd.cpp $(HDRS)
	$(CXX) -O3 -std=c++17 -fPIC -fopenmp -Wall -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) -shared --offload-arch=$(ARCH) -o $@ $(OBJS) -L/opt/rocm/lib -lrccl -fopenmp -Wl,-rpath,/opt/rocm/lib

oracle:
	$(MAKE) -C oracle

# C++ programs over the SVGDCpp-compatible headers (include/Core, Model, Kernel, Optimizer)
CPP_FLAGS := -O2 -std=c++17 -Wall -fopenmp -Iinclude
CPP_LINK := -Lsvgdcpp_amd -lsvgdcpp_amd -Wl,-rpath,'$$ORIGIN/../svgdcpp_amd' -Wl,--allow-shlib-undefined
CPP_HDRS := $(wildcard include/SVGDCpp/*.hpp include/SVGDCpp/*/*.hpp) include/Core include/Model include/Kernel include/Optimizer
CPP_BINS := build/mvn_example build/gmm_example build/svgd_run_bench build/test_api build/test_dist build/test_ksd build/test_glm build/test_glm_hess build/test_glm_predict build/test_imq build/test_ksd_imq build/test_thin build/test_mmd

cpp: $(CPP_BINS) build/host_grad_bench

# host gradient builds side by side (tools/bench_host_grad.cpp; host only)
build/host_grad_bench: tools/bench_host_grad.cpp $(SRC_DIR)/host_models.o $(SRC_DIR)/host_models.h
	@mkdir -p build
	$(CXX) -O2 -std=c++17 -fopenmp $< $(SRC_DIR)/host_models.o -o $@

build/%: examples/%.cpp $(CPP_HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CPP_FLAGS) $< -o $@ $(CPP_LINK)

build/test_api: tests/cpp/test_api.cpp $(CPP_HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CPP_FLAGS) $< -o $@ $(CPP_LINK)

build/test_dist: tests/cpp/test_dist.cpp $(CPP_HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CPP_FLAGS) $< -o $@ $(CPP_LINK)

build/test_ksd: tests/cpp/test_ksd.cpp $(CPP_HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CPP_FLAGS) $< -o $@ $(CPP_LINK)

build/test_glm: tests/cpp/test_glm.cpp $(CPP_HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CPP_FLAGS) $< -o $@ $(CPP_LINK)

build/test_glm_hess: tests/cpp/test_glm_hess.cpp $(CPP_HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CPP_FLAGS) $< -o $@ $(CPP_LINK)

build/test_glm_predict: tests/cpp/test_glm_predict.cpp $(CPP_HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CPP_FLAGS) $< -o $@ $(CPP_LINK)

build/test_imq: tests/cpp/test_imq.cpp $(CPP_HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CPP_FLAGS) $< -o $@ $(CPP_LINK)

build/test_ksd_imq: tests/cpp/test_ksd_imq.cpp $(CPP_HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CPP_FLAGS) $< -o $@ $(CPP_LINK)

build/test_thin: tests/cpp/test_thin.cpp $(CPP_HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CPP_FLAGS) $< -o $@ $(CPP_LINK)

build/test_mmd: tests/cpp/test_mmd.cpp $(CPP_HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CPP_FLAGS) $< -o $@ $(CPP_LINK)

# Host-code sanitizers (ASan + UBSan): planners (phi and median), host models and the CPU oracle
# linked into a self-checking driver (the HIP host code needs a GPU: see
# tests/cpp/sanitize_host.cpp).  Run by tests/test_sanitize.py.
SAN := -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=all
build/sanitize_host: tests/cpp/sanitize_host.cpp $(SRC_DIR)/plan.cpp $(SRC_DIR)/plan.h $(SRC_DIR)/built.h $(SRC_DIR)/median_plan.cpp $(SRC_DIR)/median_plan.h $(SRC_DIR)/select_state.h $(SRC_DIR)/host_models.cpp oracle/svgd_oracle.c
	@mkdir -p build/san
	gcc -O1 -g -std=c11 -fopenmp -ffp-contract=off $(SAN) -c oracle/svgd_oracle.c -o build/san/oracle.o
	$(CXX) -O1 -g -std=c++17 -fopenmp $(SAN) -c $(SRC_DIR)/plan.cpp -o build/san/plan.o
	$(CXX) -O1 -g -std=c++17 -fopenmp $(SAN) -c $(SRC_DIR)/median_plan.cpp -o build/san/median_plan.o
	$(CXX) -O1 -g -std=c++17 -fopenmp $(SAN) -c $(SRC_DIR)/host_models.cpp -o build/san/host_models.o
	$(CXX) -O1 -g -std=c++17 -fopenmp $(SAN) tests/cpp/sanitize_host.cpp build/san/*.o -o $@ -lm

sanitize: build/sanitize_host
	ASAN_OPTIONS=detect_leaks=1 OMP_NUM_THREADS=2 ./build/sanitize_host

# the host GLM (host_glm.cpp) under the same sanitizers, with a driver of its
# own (tests/cpp/sanitize_glm.cpp).  Run by tests/test_sanitize_glm.py.
build/sanitize_glm: tests/cpp/sanitize_glm.cpp $(SRC_DIR)/host_glm.cpp $(SRC_DIR)/host_glm.h include/svgdcpp_amd/svgd_capi.h \
        $(SRC_DIR)/ctx.h $(SRC_DIR)/resource.h $(SRC_DIR)/hostcomm.h $(SRC_DIR)/host_models.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -fopenmp $(SAN) tests/cpp/sanitize_glm.cpp $(SRC_DIR)/host_glm.cpp -o $@ -lm

sanitize_glm: build/sanitize_glm
	ASAN_OPTIONS=detect_leaks=1 OMP_NUM_THREADS=2 ./build/sanitize_glm

# the host prediction (svgd_glm_predict_host of host_glm.cpp) under the same
# sanitizers (tests/cpp/sanitize_glm_predict.cpp).  Run by
# tests/test_sanitize_glm_predict.py.
build/sanitize_glm_predict: tests/cpp/sanitize_glm_predict.cpp $(SRC_DIR)/host_glm.cpp $(SRC_DIR)/host_glm.h include/svgdcpp_amd/svgd_capi.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -fopenmp $(SAN) tests/cpp/sanitize_glm_predict.cpp $(SRC_DIR)/host_glm.cpp -o $@ -lm

sanitize_glm_predict: build/sanitize_glm_predict
	ASAN_OPTIONS=detect_leaks=1 OMP_NUM_THREADS=2 ./build/sanitize_glm_predict

# the host IMQ phi (host_imq.cpp) under the same sanitizers
# (tests/cpp/sanitize_imq.cpp).  Run by tests/test_sanitize_imq.py.
build/sanitize_imq: tests/cpp/sanitize_imq.cpp $(SRC_DIR)/host_imq.cpp include/svgdcpp_amd/svgd_capi.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -fopenmp $(SAN) tests/cpp/sanitize_imq.cpp $(SRC_DIR)/host_imq.cpp -o $@ -lm

sanitize_imq: build/sanitize_imq
	ASAN_OPTIONS=detect_leaks=1 OMP_NUM_THREADS=2 ./build/sanitize_imq

# the host KSD of both kernels (host_ksd.cpp) under the same sanitizers
# (tests/cpp/sanitize_ksd.cpp).  Run by tests/test_sanitize_ksd.py.
build/sanitize_ksd: tests/cpp/sanitize_ksd.cpp $(SRC_DIR)/host_ksd.cpp include/svgdcpp_amd/svgd_capi.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -fopenmp $(SAN) tests/cpp/sanitize_ksd.cpp $(SRC_DIR)/host_ksd.cpp -o $@ -lm

sanitize_ksd: build/sanitize_ksd
	ASAN_OPTIONS=detect_leaks=1 OMP_NUM_THREADS=2 ./build/sanitize_ksd

# the host Stein thinning (host_thin.cpp) under the same sanitizers
# (tests/cpp/sanitize_thin.cpp).  Run by tests/test_sanitize_thin.py.
build/sanitize_thin: tests/cpp/sanitize_thin.cpp $(SRC_DIR)/host_thin.cpp include/svgdcpp_amd/svgd_capi.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -fopenmp $(SAN) tests/cpp/sanitize_thin.cpp $(SRC_DIR)/host_thin.cpp -o $@ -lm

sanitize_thin: build/sanitize_thin
	ASAN_OPTIONS=detect_leaks=1 OMP_NUM_THREADS=2 ./build/sanitize_thin

# the host MMD (host_mmd.cpp) under the same sanitizers
# (tests/cpp/sanitize_mmd.cpp).  Run by tests/test_sanitize_mmd.py.
build/sanitize_mmd: tests/cpp/sanitize_mmd.cpp $(SRC_DIR)/host_mmd.cpp include/svgdcpp_amd/svgd_capi.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -fopenmp $(SAN) tests/cpp/sanitize_mmd.cpp $(SRC_DIR)/host_mmd.cpp -o $@ -lm

sanitize_mmd: build/sanitize_mmd
	ASAN_OPTIONS=detect_leaks=1 OMP_NUM_THREADS=2 ./build/sanitize_mmd

clean:
	rm -f $(OBJS) $(LIB) $(CPP_BINS) build/sanitize_host build/sanitize_glm build/sanitize_glm_predict build/sanitize_imq build/sanitize_ksd build/sanitize_thin build/sanitize_mmd
	$(MAKE) -C oracle clean

.PHONY: all oracle cpp clean sanitize sanitize_glm sanitize_glm_predict sanitize_imq sanitize_ksd sanitize_thin sanitize_mmd print-objs
