# Builds tests/c/_bin/test_chacha_vtable: the ChaCha20-Poly1305 picotls objects of the MI355X engine driven through
# picotls' own core side by side with ptls_openssl_chacha20poly1305 / ptls_openssl_chacha20 (lib/picotls.c and
# lib/openssl.c in oracle/_ref/libtls12_ref.so, which links libcrypto). Run as `make -f chacha.mk` in this directory.
# Needs picotls headers at build time (PICOTLS_INCLUDE); the binary travels to the GPU box with the repo snapshot.
ROOT := $(abspath $(CURDIR)/../..)
PICOTLS_INCLUDE ?= /root/reference/include
OUT := $(CURDIR)/_bin

all: $(OUT)/test_chacha_vtable

$(OUT)/test_chacha_vtable: test_chacha_vtable.c $(ROOT)/include/picotls/mi355x_chacha20_picotls.h $(ROOT)/include/picotls/mi355x_chacha20.h $(ROOT)/picotls_amd/_lib/libptls_mi355x_picotls.so $(ROOT)/oracle/_ref/libtls12_ref.so
	mkdir -p $(OUT)
	gcc -std=gnu99 -O2 -Wall -mavx2 -maes -mpclmul -I$(ROOT)/include -I$(PICOTLS_INCLUDE) -o $@ test_chacha_vtable.c \
	    -L$(ROOT)/oracle/_ref -ltls12_ref -L$(ROOT)/picotls_amd/_lib -lptls_mi355x_picotls -lptls_mi355x \
	    -Wl,-rpath,'$$ORIGIN/../../../oracle/_ref' -Wl,-rpath,'$$ORIGIN/../../../picotls_amd/_lib' -lpthread

.PHONY: all
