"""Build the gfx950 C-ABI library in-tree:  ao_amd/_C_mi355.so

    python -m ao_amd.build            # rebuild if sources are newer
    python -m ao_amd.build --force

hipcc cross-compiles for gfx950 without a GPU.  The .so is git-ignored but
travels with the gpurun snapshot.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "_C_mi355.so")
OPS_LIB = os.path.join(HERE, "_C_mi355_ops.so")  # C++ dispatcher registrations (csrc_torch/binding.cpp), links against LIB
OPS_SRC = os.path.join(HERE, "csrc_torch", "binding.cpp")
OPS_SRC_STABLE = os.path.join(HERE, "csrc_torch", "binding_stable.cpp")  # torchao:: ops through the stable ABI (no ATen / c10 headers)
CXX = os.environ.get("CXX", "g++")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    "-fPIC",
    "-shared",
    "-fno-strict-aliasing",
    # the loop vectorizer "vectorises" wave-uniform scalar loops across SGPRs (8x unrolled unit
    # search, 480 SGPR spills in the streaming GEMV); nothing here wants it
    "-fno-vectorize",
    "-Wno-unused-result",
]
# Flags of single sources.  nvfp4_grouped_train_kernels.hip is compiled without packed fp32 VALU operations (v_pk_add / mul / fma_f32):
# its fp32 arithmetic is quant_math.h's chain of single operations, and the packed pairing of the two 16-point Hadamard transforms a lane
# holds costs registers instead of saving issue slots -- nvfp4_train_group_amax_kernel takes 84 VGPRs (5 waves a SIMD) with them and 61
# (8 waves) without, nvfp4_wgrad_kernel 88 and 86.  It is a cc1 feature switch that a compiler may stop honouring without failing the
# build: the check is the resource report (-Rpass-analysis=kernel-resource-usage), 61 and 86 VGPRs.
# attention_kernels.hip likewise: its fp32 work is the softmax's single multiplies, subtractions and v_exp_f32 between two MFMA products.
# bitnet_kernels.hip likewise: its fp32 work is the casts' chain of single IEEE operations and a two-multiply epilogue.
# intx_kernels.hip likewise: the affine cast's chain of single operations and the decode's add and multiply per weight.
# codebook_kernels.hip likewise: the score is quant_math.h's chain of single v_fma_f32 in index order, the decode one multiply per weight.
# With packed operations allowed the compiler pairs the rows a lane holds and codebook_assign_kernel grows: 256 VGPRs against 212 at d = 8,
# k = 16 and 204 against 124 at d = 4, k = 16 (the 16-entry table is kept in registers across tiles either way), 106 against 68 for the Lloyd
# step at d = 8, k = 256 (4 waves a SIMD against 7).  The resource report of this source is the check, as above; the two builds were not
# timed against each other.
# da8w4_kernels.hip likewise: the casts' chain of single operations and one v_fma_f32 a register at a group boundary.
_NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
SOURCE_FLAGS = {
    "nvfp4_grouped_train_kernels.hip": _NO_PACKED_FP32,
    "attention_kernels.hip": _NO_PACKED_FP32,
    "bitnet_kernels.hip": _NO_PACKED_FP32,
    "intx_kernels.hip": _NO_PACKED_FP32,
    "codebook_kernels.hip": _NO_PACKED_FP32,
    "da8w4_kernels.hip": _NO_PACKED_FP32,
}


def sources():
    return sorted(
        os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip")
    )


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = sources() + [
        os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")
    ] + [os.path.join(os.path.dirname(HERE), "include", "ao_mi355.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build_ops(force=False, verbose=False):
    """Compile the host-only dispatcher binding against the installed torch (no device code: plain g++)."""
    if not force and os.path.exists(OPS_LIB) and os.path.getmtime(OPS_LIB) >= max(os.path.getmtime(OPS_SRC), os.path.getmtime(OPS_SRC_STABLE), os.path.getmtime(LIB)):
        return OPS_LIB
    import torch

    t = os.path.dirname(torch.__file__)
    cmd = [CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}",
           f"-I{t}/include", f"-I{t}/include/torch/csrc/api/include", "-I/opt/rocm/include", OPS_SRC, OPS_SRC_STABLE, "-o", OPS_LIB,
           f"-L{t}/lib", "-lc10", "-ltorch_cpu", "-ltorch", "-lc10_hip", "-ltorch_hip", f"-L{HERE}", "-l:_C_mi355.so",
           "-Wl,-rpath,$ORIGIN", f"-Wl,-rpath,{t}/lib"]
    if verbose:
        print(" ".join(cmd))
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if out.returncode != 0:
        raise RuntimeError(f"building {OPS_LIB} failed:\n{out.stdout.decode()}")
    return OPS_LIB


def _prune_objects(bdir, keep):
    """Objects of sources that no longer exist must not linger (they never ship -- ao_amd/build/ is gpurun-ignored -- but a
    stale object is a stale object)."""
    for f in os.listdir(bdir):
        p = os.path.join(bdir, f)
        if f.endswith(".o") and p not in keep:
            os.remove(p)


def build(force=False, verbose=False, lab=False):
    """Compile every .hip under ao_amd/csrc into one shared library, then the dispatcher binding.  lab=True: the laboratory
    library instead (tools/bin/_C_mi355_lab.so, -DAO_LAB: the product plus the wrong-result ablation builds of the profiling
    tools; select it with AO_MI355_LIB=tools/bin/_C_mi355_lab.so) -- never what ao_amd loads by default."""
    if lab:
        return _build_lab(verbose)
    if not force and not _stale():
        build_ops(force=False, verbose=verbose)
        return LIB
    objs = []
    procs = []
    bdir = os.path.join(HERE, "build")
    os.makedirs(bdir, exist_ok=True)
    for src in sources():
        obj = os.path.join(bdir, os.path.basename(src) + ".o")
        cmd = [HIPCC] + [f for f in FLAGS if f != "-shared"] + SOURCE_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        objs.append(obj)
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{out.decode()}")
    _prune_objects(bdir, set(objs))
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if out.returncode != 0:
        raise RuntimeError(f"link failed:\n{out.stdout.decode()}")
    build_ops(force=True, verbose=verbose)
    return LIB


def _build_lab(verbose=False):
    out = os.path.join(os.path.dirname(HERE), "tools", "bin", "_C_mi355_lab.so")
    bdir = os.path.join(HERE, "build", "lab")
    os.makedirs(bdir, exist_ok=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    objs, procs = [], []
    for src in sources():
        obj = os.path.join(bdir, os.path.basename(src) + ".o")
        cmd = [HIPCC] + [f for f in FLAGS if f != "-shared"] + SOURCE_FLAGS.get(os.path.basename(src), []) + ["-DAO_LAB=1", "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        objs.append(obj)
    for src, p in procs:
        o, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{o.decode()}")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout.decode()}")
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True, lab="--lab" in sys.argv))
