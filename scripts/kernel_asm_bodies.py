#!/usr/bin/env python3
"""One line per kernel of gfx950 assembly files: a hash of the instruction stream and of the kernel descriptor.

    cd robustvlm_amd/csrc
    hipcc -O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -S --cuda-device-only attention_bf16.hip -o new.s
    python3 ../../scripts/kernel_asm_bodies.py old.s > old.txt; python3 ../../scripts/kernel_asm_bodies.py new.s > new.txt
    diff old.txt new.txt

Two builds of a kernel have the same body hash exactly when their assembly agrees up to symbol names, the function number
in local labels and comments: the check that a source-level change (moved code, a helper, a deleted constant-false arm) left
the kernel alone.  Template arguments are part of the printed name, so a kernel that lost one shows as a renamed line with
equal hashes.  scripts/kernel_symbol_sizes.sh answers the coarser question from built objects.
"""
import hashlib
import re
import sys


def norm(line):
    line = line.split(";", 1)[0].rstrip()
    line = re.sub(r"_Z\w+", "SYM", line)
    return re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+", r".L\1", line)


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:12]


def kernels(path):
    text = open(path).read().split("\n")
    desc, body = {}, {}
    for i, line in enumerate(text):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            end = next(j for j in range(i, len(text)) if ".end_amdhsa_kernel" in text[j])
            desc[m.group(1)] = [norm(t).strip() for t in text[i + 1:end]]
    for sym in desc:
        start = next(j for j, t in enumerate(text) if t.startswith(sym + ":"))
        end = next(j for j in range(start, len(text)) if ".amdhsa_kernel" in text[j])
        body[sym] = [t for t in (norm(t) for t in text[start + 1:end]) if t.strip()]
    return desc, body


def pretty(sym):     # _ZN4rvlm15attn_fwd_kernelILb1ELi5EEEv... -> attn_fwd_kernel<1,5>
    m = re.match(r"_ZN\d+[a-z]+(\d+)", sym)
    if not m:
        return sym
    name, rest = sym[m.end():m.end() + int(m.group(1))], sym[m.end() + int(m.group(1)):]
    t = re.match(r"I((?:L[a-z]\d+E)+)E", rest)
    return name + ("<" + ",".join(re.findall(r"L[a-z](\d+)E", t.group(1))) + ">" if t else "")


def field(desc, key):
    return next((t.split()[-1] for t in desc if t.startswith(key + " ")), "?")


rows = []
for path in sys.argv[1:]:
    desc, body = kernels(path)
    for sym in desc:
        rows.append(f"{pretty(sym)}  body {digest(body[sym])} ({len(body[sym])} lines)  descriptor {digest(desc[sym])}"
                    f"  vgpr {field(desc[sym], '.amdhsa_next_free_vgpr')} sgpr {field(desc[sym], '.amdhsa_next_free_sgpr')}"
                    f" scratch {field(desc[sym], '.amdhsa_private_segment_fixed_size')}"
                    f" lds {field(desc[sym], '.amdhsa_group_segment_fixed_size')}")
print("\n".join(sorted(rows)))
