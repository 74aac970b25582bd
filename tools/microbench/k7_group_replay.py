"""Development tool: the issue ceiling of K7's OWN instruction mix.

Takes the 4-entry group body of `blend_backward_kernel<false, false, false>` (FAST, SEG, DEPTH) exactly as hipcc emits it for the product
(`gaussianeditor_amd/csrc/gsr_blend.hip`, the inner loop of backward_tile: footprints + exp of four entries, the
transmittance / colour recurrences, the nine moments, the 4-entry transposed wave reduction and the nine ds_add_f32),
strips its control flow (the `no lane contributes` skip and the loop's own back edge), and replays it REP times per wave
from zero-initialised registers and LDS -- no global memory, no barrier, no list walk.  Launched as 4-wave workgroups (one
wave per SIMD, like the product) with 1 .. 4 workgroups per CU on every CU, it measures how many cycles a SIMD needs per
group when 1 .. 4 waves share it: THAT, not a per-instruction figure, is the ceiling of K7's instruction mix (round 6: 835
cycles per group and SIMD at four waves, profiles/r06_b_k7_limiter.md).  Variants: `full` (as compiled), `nolds` (every ds_* instruction and the waits for
them removed: the VALU/SALU stream alone), `noxlane` (additionally without the permlane / DPP reduction steps).

    python tools/microbench/k7_group_replay.py            # writes build_variants/k7_group_replay.hip and builds it (no GPU needed)
    build_variants/k7_group_replay                        # on the MI355X: prints one table (and JSON with --json)
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "build_variants")
KERNEL = "_ZN3gsr21blend_backward_kernelILb0ELb0ELb0ELb0ELb0EEEvNS_9BlendArgsE"
FLAGS = ("--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -munsafe-fp-atomics -fno-gpu-rdc -fno-slp-vectorize "
         "-fvisibility=hidden -mllvm -amdgpu-sched-strategy=max-ilp -mllvm -amdgpu-atomic-optimizer-strategy=None").split()


def product_isa(extra=()) -> str:
    os.makedirs(OUT, exist_ok=True)
    s = os.path.join(OUT, "gsr_blend.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", *FLAGS, *extra, "-S", "--cuda-device-only", "-o", s,
                           os.path.join(ROOT, "gaussianeditor_amd", "csrc", "gsr_blend.hip")], stderr=subprocess.DEVNULL)
    return open(s).read()


def group_body(isa: str):
    """The first depth-2 loop of the kernel that holds the transposed reduction: lines from its header label to the jump
    back, in program order, plus the two join blocks behind it (exec restore, loop increment)."""
    lines = isa.split("\n")
    a = next(i for i, ln in enumerate(lines) if ln.startswith(KERNEL + ":"))
    b = next(i for i in range(a, len(lines)) if lines[i].startswith("\t.end_amdhsa_kernel") or lines[i].startswith(".Lfunc_end"))
    k = lines[a:b]
    heads = [i for i, ln in enumerate(k) if "Inner Loop Header: Depth=2" in ln]
    is_label = lambda ln: re.match(r"^\.LBB\d+_\d+:", ln) is not None  # noqa: E731
    for h in heads:
        j = h
        while not is_label(k[j]):  # the loop's label: the header comment's own line, or the one in front of it
            j -= 1
        end = next(i for i in range(j + 1, len(k)) if is_label(k[i]) and "Depth=2" not in k[i])
        # the loop's join blocks (exec restore, increment + back edge) are emitted IN FRONT of the header: the run of
        # labels marked "Depth=2" that ends at the header
        start = j
        for i in range(j - 1, -1, -1):
            if is_label(k[i]):
                if "Depth=2" not in k[i]:
                    break
                start = i
        if any("v_permlane32_swap" in ln for ln in k[j:end]):
            return k[j].split(":")[0], k[start:j], k[j:end]
    raise SystemExit("group loop not found in the ISA")


def clean(lines, variant):
    out = []
    for ln in lines:
        t = ln.split(";")[0].rstrip()
        if not t.strip() or t.strip().startswith("."):
            continue
        t = t.strip()
        op = t.split()[0]
        if op in ("s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_execz", "s_cbranch_execnz", "s_cbranch_scc1", "s_cbranch_scc0", "s_branch"):
            continue  # straight line: every group is evaluated in full, the masked tail included
        m = re.match(r"v_add_u32_e32 (v\d+), 64, \1$", t)
        if m:
            t = f"v_add_u32_e32 {m.group(1)}, 0, {m.group(1)}"  # (the LDS cursor of the loop: stays on the first group's records)
        if variant in ("nolds", "noxlane"):
            if op.startswith("ds_"):
                continue
            if op == "s_waitcnt" and "lgkmcnt" in t and "vmcnt" not in t:
                continue
        if variant == "noxlane" and (op.startswith("v_permlane") or op.endswith("_dpp")):
            continue
        if op == "s_waitcnt" and "vmcnt" in t and "lgkmcnt" not in t:
            continue  # (no vector memory in the replay)
        out.append(t)
    return out


def packed_lanes(nm=9, group=4):
    """wave_sum4_pack's lane map (pack_lanes<NM>, gsr_blend.hip), emulated: -> (mask of the lanes that add, [moment of lane])."""
    t = [[k] * 64 for k in range(nm * group)]
    for s in (8, 4, 2, 1, 32, 16):
        out = [[(b if i & s else a)[i] for i in range(64)] for a, b in zip(t[0::2], t[1::2])]
        t = out + ([t[-1]] if len(t) & 1 else [])
    assert len(t) == 1
    seen, mask = set(), 0
    for i, val in enumerate(t[0]):
        if val not in seen:
            mask |= 1 << i
        seen.add(val)
    assert len(seen) == nm * group
    return mask, [val // group for val in t[0]]


def registers(body):
    v, s = set(), set()
    for t in body:
        for m in re.finditer(r"\bv\[(\d+):(\d+)\]", t):
            v.update(range(int(m.group(1)), int(m.group(2)) + 1))
        for m in re.finditer(r"\bv(\d+)\b", t):
            v.add(int(m.group(1)))
        for m in re.finditer(r"\bs\[(\d+):(\d+)\]", t):
            s.update(range(int(m.group(1)), int(m.group(2)) + 1))
        for m in re.finditer(r"\bs(\d+)\b", t):
            s.add(int(m.group(1)))
    return sorted(v), sorted(s)


def emit(isa: str) -> str:
    label, join, loop = group_body(isa)
    variants = {}
    for name in ("full", "nolds", "noxlane"):
        body = clean(loop, name) + clean(join, name)
        variants[name] = body
    v, s = registers(variants["full"])
    cnt = max(r for r in range(96) if r not in s)  # loop counter SGPR, outside the body's set (s100+ are reserved)
    src = ['// GENERATED by tools/microbench/k7_group_replay.py from the product\'s ISA -- do not edit.',
           '#include <hip/hip_runtime.h>', '#include <cstdint>', '#include <cstdio>', '#include <cstring>', '#include <vector>', '']
    for name, body in variants.items():
        n_valu = sum(1 for t in body if t.startswith("v_"))
        n_salu = sum(1 for t in body if t.startswith("s_") and not t.startswith("s_waitcnt"))
        n_lds = sum(1 for t in body if t.startswith("ds_"))
        init = [f"v_mov_b32 v{r}, 0" for r in v] + [f"s_mov_b32 s{r}, 0" for r in s]
        # what the masked tail runs under (the operand of its s_and_saveexec_b64): the lanes that add a total -- lane 15 of every
        # row with one row_shr chain per moment, the lowest lane of every total with the packed reduction (told by its
        # row_ror:8)
        tail = next(re.match(r"s_and_saveexec_b64 s\[\d+:\d+\], s\[(\d+):(\d+)\]", t) for t in body if t.startswith("s_and_saveexec_b64"))
        packed = any("row_ror:8" in t for t in variants["full"])
        mask, term = packed_lanes() if packed else (0x8000800080008000, None)
        init += [f"s_mov_b32 s{tail.group(1)}, {mask & 0xffffffff:#x}", f"s_mov_b32 s{tail.group(2)}, {mask >> 32:#x}", f"s_mov_b32 s{cnt}, %0"]
        if packed:
            # the lane's own share of the add's address, 4 x its moment: the addend of the v_mad_u64_u32 in front of the single
            # ds_add_f32.  (All four entries of the replayed group are null records, slot 0: the four lanes of a moment add to
            # one address, as the four row ends of the unpacked form do.)
            mad = next(re.match(r"v_mad_u64_u32 v\[\d+:\d+\], s\[\d+:\d+\], v\d+, \d+, v\[(\d+):\d+\]", t) for t in variants["full"]
                       if t.startswith("v_mad_u64_u32"))
            init += [f"v_writelane_b32 v{mad.group(1)}, {4 * k}, {i}" for i, k in enumerate(term)]
        text = init + [f"K7R_{name}_%=:"] + body + [f"s_sub_u32 s{cnt}, s{cnt}, 1", f"s_cmp_lg_u32 s{cnt}, 0", f"s_cbranch_scc1 K7R_{name}_%="]
        asm = "\n".join(f'      "{t}\\n"' for t in text)
        clob = ", ".join([f'"v{r}"' for r in v] + [f'"s{r}"' for r in s] + [f'"s{cnt}"', '"vcc"', '"scc"', '"memory"'])
        src += [f"// {name}: {n_valu} VALU + {n_salu} SALU + {n_lds} LDS instructions per group of four entries",
                f"constexpr int N_{name}[3] = {{{n_valu}, {n_salu}, {n_lds}}};",
                f"__global__ void __launch_bounds__(256) replay_{name}(uint64_t* cyc, int rep) {{",
                "  __shared__ float lds[5120];  // 20 KB, as the product's workgroup; zero: slot 0, null records",
                "  for (int i = threadIdx.x; i < 5120; i += 256) lds[i] = 0.f;",
                "  __syncthreads();",
                "  const uint64_t t0 = __builtin_amdgcn_s_memtime();",
                "  asm volatile(", asm, f"      : : \"s\"(rep) : {clob});",
                "  const uint64_t t1 = __builtin_amdgcn_s_memtime();",
                "  if ((threadIdx.x & 63) == 0) cyc[blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;",
                "  if (rep < 0) lds[threadIdx.x] = 1.f;", "}", ""]
    src += [r'''
template <class K>
static void run(const char* name, K kern, const int n[3], int cus, bool json) {
  const int rep = 4000;
  for (int wgs = 1; wgs <= 5; ++wgs) {
    const int grid = cus * wgs;
    uint64_t* cyc;
    (void)hipMalloc(&cyc, sizeof(uint64_t) * grid * 4);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, 0, cyc, rep);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, 0, cyc, rep);
    (void)hipDeviceSynchronize();
    std::vector<uint64_t> h(grid * 4);
    (void)hipMemcpy(h.data(), cyc, sizeof(uint64_t) * grid * 4, hipMemcpyDeviceToHost);
    double mean = 0;
    uint64_t mx = 0;
    for (auto v : h) { mean += (double)v; mx = v > mx ? v : mx; }
    mean /= (double)h.size();
    const double per_wave = mean / rep, per_simd = per_wave / wgs, instr = n[0] + n[1] + n[2];
    if (json)
      printf("{\"variant\": \"%s\", \"waves_per_simd\": %d, \"cycles_per_group_wave\": %.1f, \"cycles_per_group_simd\": %.1f, "
             "\"cycles_per_instr_simd\": %.3f, \"valu\": %d, \"salu\": %d, \"lds\": %d, \"max_over_mean\": %.3f}\n",
             name, wgs, per_wave, per_simd, per_simd / instr, n[0], n[1], n[2], (double)mx / rep / per_wave);
    else
      printf("%-8s %d waves/SIMD: %8.1f cycles per group and wave, %7.1f per group and SIMD = %5.2f cycles per instruction "
             "(%d VALU + %d SALU + %d LDS), slowest wave %.3f x mean\n",
             name, wgs, per_wave, per_simd, per_simd / instr, n[0], n[1], n[2], (double)mx / rep / per_wave);
    fflush(stdout);
    (void)hipFree(cyc);
  }
}

int main(int argc, char** argv) {
  const bool json = argc > 1 && !strcmp(argv[1], "--json");
  hipDeviceProp_t p;
  (void)hipGetDeviceProperties(&p, 0);
  const int cus = p.multiProcessorCount;
  if (!json) printf("%s, %d CUs; 4-wave workgroups (one wave per SIMD), 1 .. 5 workgroups per CU, 4000 groups per wave\n", p.name, cus);
  run("full", replay_full, N_full, cus, json);
  run("nolds", replay_nolds, N_nolds, cus, json);
  run("noxlane", replay_noxlane, N_noxlane, cus, json);
  return 0;
}
''']
    return "\n".join(src)


def main():
    # optional: NAME followed by extra compiler flags for the product source, e.g. `noilp -mllvm -amdgpu-sched-strategy=max-occupancy`
    name = "k7_group_replay" + ("_" + sys.argv[1] if len(sys.argv) > 1 else "")
    isa = product_isa(sys.argv[2:])
    hip = os.path.join(OUT, name + ".hip")
    open(hip, "w").write(emit(isa))
    exe = os.path.join(OUT, name)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-Wno-unused-value", hip, "-o", exe])
    print("built", exe)


if __name__ == "__main__":
    main()
