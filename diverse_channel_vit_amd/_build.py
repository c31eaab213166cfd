"""Builds libdcv_hip.so (gfx950 only) from csrc/*.hip with hipcc.  In-tree, so the .so travels with
the repo snapshot to the GPU box.  `python -m diverse_channel_vit_amd._build` or __graft_entry__.build()."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libdcv_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=fast", "-Wall"]
# per-file extras.  attn: keep MFMA accumulators in arch VGPRs (gfx950's register file is unified) — the
# softmax touches them with VALU every tile and the AGPR form costs ~250 v_accvgpr moves per key tile.
EXTRA = {"attn.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
         # backward: additionally no SLP vectorizer — its v_pk_* packing of the dS arithmetic costs 48 register-pair moves per tile
         # (dK/dV kernel 4 % slower); the forward keeps it (its packed forms are written out and measured 2 % faster)
         "attn_bwd.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1", "-fno-slp-vectorize"],
         # third dK/dV form: its MFMAs are inline asm with explicit register classes; the flag keeps hipcc's own choices out of the accumulator file
         "attn_bwd3.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1", "-fno-slp-vectorize"]}


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


#: diagnostic translation units that REPLACE a product source in a variant build.  A twin is kept only while it builds and the resulting library still
#: carries every entry of hip.EXPORTS; the one left holds the -DDCV_K3_ABL=<mask> timing-only ablations and the -DDCV_K3_STAMP cycle stamps of the
#: persistent dK/dV kernel (the twins of gemm.hip, attn.hip and attn_bwd.hip had fallen behind the product sources and were removed)
INSTRUMENTED = {"attn_bwd3.hip": os.path.join(HERE, "..", "tools", "probes", "attn_bwd3_instrumented.hip")}


def build_variant(name: str, defines, verbose: bool = True, flags=(), instrumented=()) -> str:
    """A/B build of the same ABI with extra -D flags -> libdcv_hip_<name>.so (select it with DCV_LIB=...).
    instrumented: product sources to replace by their diagnostic twin (INSTRUMENTED), e.g. ("attn_bwd3.hip",) for -DDCV_K3_ABL=n."""
    objdir = os.path.join(HERE, "build", "variant_" + name)
    os.makedirs(objdir, exist_ok=True)
    objs = []
    for src in sources():
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        base = os.path.basename(src)
        if base in instrumented:
            src = os.path.abspath(INSTRUMENTED[base])
        cmd = [HIPCC] + FLAGS + EXTRA.get(base, []) + list(flags) + ["-I" + CSRC] + ["-D" + d for d in defines] + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
        objs.append(obj)
    lib = os.path.join(HERE, f"libdcv_hip_{name}.so")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stderr}")
    if verbose:
        print("built", lib)
    return lib


def build(force: bool = False, verbose: bool = True) -> str:
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(HERE, "..", "include", "dcv.h")]
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    for src in sources():
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        if force or _stale(obj, [src, os.path.abspath(__file__)] + hdrs):
            jobs.append((src, obj))

    def cc(job):
        src, obj = job
        cmd = [HIPCC] + FLAGS + EXTRA.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)
        return obj

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(cc, jobs))
    objs = [os.path.join(objdir, os.path.basename(s)[:-4] + ".o") for s in sources()]
    if force or jobs or _stale(LIB, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    if verbose:
        print(f"built {LIB} ({len(jobs)} object(s) recompiled)")
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
