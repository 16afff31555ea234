#!/bin/bash
# development aid: register / scratch / LDS use of every kernel of one translation unit (hipcc resource-usage remarks)
# usage: scripts/kres.sh [TU.hip] [extra hipcc flags]     TU: a path, or a name in ppcseq_amd/csrc (also KRES_SRC=...)
#   the engine's kernels are one family per file -- ppcx_kernels.hip (LDS-staged log-likelihood), ppcx_kernels_stream.hip,
#   ppcx_kernels_ls.hip (merged launch, step, update, ADVI), ppcx_kernels_close.hip, ppcx_kernels_model.hip;
#   default: ppcx_kernels.hip. All of them: for f in ppcseq_amd/csrc/ppcx_kernels*.hip; do scripts/kres.sh $f; done
src="${KRES_SRC:-ppcseq_amd/csrc/ppcx_kernels.hip}"
case "$1" in *.hip) src="$1"; shift;; esac
[ -f "$src" ] || src="ppcseq_amd/csrc/$src"
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -c -Rpass-analysis=kernel-resource-usage "$@" "$src" -o /tmp/kres.o 2>&1 \
 | grep -E "Function Name|TotalSGPRs|VGPRs:|Spill|ScratchSize|Occupancy|LDS Size" | sed -E 's/.*remark: [^ ]+ +//; s/ \[-Rpass.*//' | paste - - - - - - - - \
 | awk -F'\t' '{n=$1; sub(/Function Name: /,"",n); printf "%-62s %s | %s | %s | %s | %s | %s\n", substr(n,1,62), $3,$4,$5,$6,$7,$8}'
