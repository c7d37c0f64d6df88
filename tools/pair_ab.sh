#!/bin/bash
# A/B of the pair-fold handshake (gram_sk.hip), alternating, host_csc per solve, over builds of tools/build_variants.sh:
#   pair_shipped   ""                        relaxed (write-through) producer, acquire fence on the consumer
#   pair_formal    "-DPMT_SK_PAIR_FORMAL=1"  plain stores -> barrier -> RELEASE flag store; relaxed spin -> ACQUIRE fence -> barrier -> plain loads
# (the other two forms of profiles/r05_pair_fold.txt, relaxed on both sides and release without the acquire, are no longer in the source)
for rep in 1 2 3; do
  for v in "$@"; do
    echo "[$rep] $v: $(PMT_LIB_PATH=$PWD/parametron.jl_amd/lib_variants/$v.so python tools/host_api_bench.py 30 2>/dev/null | grep -E '"handoff_host_csc"|"c3_host_csc"|"handoff_device"' | tr -d '\n')"
  done
done
