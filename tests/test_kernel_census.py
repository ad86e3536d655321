"""Which filter-bank kernels the product library ships (CPU: reads the built libraries' gfx950 code objects, runs nothing).

libpbd_hip.so holds the k_conv* kernels a product handle can launch and no other; the measured-and-dropped variants
(k_conv_variants.hip, k_conv_split_variants.hip) are in the tuning and probe libraries only.  Names and resource counts come from
the code objects' metadata notes (.name, .vgpr_spill_count, .sgpr_spill_count, .private_segment_fixed_size), read with the LLVM
tools that ship with ROCm; no instruction is inspected."""
import glob
import os
import re
import shutil
import subprocess


from partsbaseddetector_amd import capi

# k_conv.hip: the exact banks (float 5x5, double 5x5 with 4 filter groups per workgroup, run-time size x {uniform, mixed-bank group}) and
# k_conv_mfma16<T, KH, KW, NHALF, WPE, NTW, B4, MIX> in its default configuration per scalar type: 5x5, run-time size, mixed-bank group
LAUNCHABLE = {
    "k_conv_exact<5,5>",
    "k_conv_exact_f64<5,5,4>",
    "k_conv_exact_generic<float,false>", "k_conv_exact_generic<float,true>",
    "k_conv_exact_generic<double,false>", "k_conv_exact_generic<double,true>",
    "k_conv_mfma16<float,5,5,2,3,2,true,false>", "k_conv_mfma16<float,0,0,2,3,2,true,false>", "k_conv_mfma16<float,0,0,2,3,2,true,true>",
    "k_conv_mfma16<double,5,5,4,2,1,true,false>", "k_conv_mfma16<double,0,0,4,2,1,true,false>", "k_conv_mfma16<double,0,0,4,2,1,true,true>",
}
# k_conv_split.hip: k_conv_split32<NT, NW = 4, PIN = 2, NS, MIX> — 1..5 n-tiles per workgroup (groups of five and every remainder), three
# bfloat16 parts / two binary16 parts, uniform bank / mixed-bank group (the filter size is a run-time argument of every form)
LAUNCHABLE |= {f"k_conv_split32<{nt},4,2,{ns},{mix}>" for nt in (1, 2, 3, 4, 5) for ns in (3, 2) for mix in ("false", "true")}


def _llvm_tool(name):
    roots = [os.environ.get("ROCM_PATH") or "/opt/rocm"]
    for r in roots:
        for sub in ("lib/llvm/bin", "llvm/bin"):
            p = os.path.join(r, sub, name)
            if os.path.exists(p):
                return p
    raise AssertionError(f"{name} not found under {roots}")


def _readable(mangled):
    """_Z<n><name>I<args>E... -> name<args> for the argument kinds these kernels use (f, d, Li<n>E, Lb<0|1>E); no template: the name"""
    m = re.match(r"_Z(N13conv_variants)?(\d+)", mangled)   # (the variants units keep their instantiations in a namespace)
    n = int(m.group(2))
    name, rest = ("conv_variants::" if m.group(1) else "") + mangled[m.end():m.end() + n], mangled[m.end() + n:]
    if not rest.startswith("I"):
        return name
    args, rest = [], rest[1:]
    while not rest.startswith("E"):
        m = re.match(r"(f)|(d)|Li(\d+)E|Lb([01])E", rest)
        assert m, f"template argument not understood in {mangled}"
        args.append("float" if m.group(1) else "double" if m.group(2) else m.group(3) if m.group(3) else ("false", "true")[int(m.group(4))])
        rest = rest[m.end():]
    return f"{name}<{','.join(args)}>"


def _conv_kernels(lib_path, tmp):
    """{readable name: (spilled VGPRs, spilled SGPRs, scratch bytes)} of the k_conv* kernels in the library's gfx950 code objects"""
    os.makedirs(tmp)
    local = shutil.copy(lib_path, tmp)   # llvm-objdump --offloading writes the bundles' entries beside its input
    subprocess.run([_llvm_tool("llvm-objdump"), "--offloading", os.path.basename(local)], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
    objs = glob.glob(os.path.join(tmp, "*gfx950"))
    assert objs, "no gfx950 code object in " + lib_path
    out = {}
    for o in objs:
        notes = subprocess.run([_llvm_tool("llvm-readobj"), "--notes", o], check=True, capture_output=True, text=True).stdout
        assert "amdhsa.kernels:" in notes, "no kernel metadata note in " + o
        # the note is YAML: `amdhsa.kernels:` is a list of maps, one `  - ` item per kernel, the kernel's own keys at four columns
        # (its arguments' keys, a `.name` among them, sit deeper); each key is looked up by itself, in whatever order they come
        for item in re.split(r"^  - ", notes.split("amdhsa.kernels:", 1)[1].split("\namdhsa.", 1)[0], flags=re.M)[1:]:
            item = "    " + item

            def field(key):
                m = re.search(rf"^    \.{key}:\s+(\S+)\s*$", item, re.M)
                assert m, f"no .{key} in a kernel's metadata of {o}:\n{item[:400]}"
                return m.group(1)

            mangled = field("name").strip("'\"")
            if not re.match(r"_Z(?:N13conv_variants)?\d+k_conv", mangled):
                continue
            name = _readable(mangled)
            assert name not in out, f"{name} twice in {lib_path}"
            out[name] = (int(field("vgpr_spill_count")), int(field("sgpr_spill_count")), int(field("private_segment_fixed_size")))
    return out


def test_product_library_holds_launchable_conv_kernels_only(tmp_path):
    got = _conv_kernels(os.path.join(os.path.dirname(capi.__file__), "libpbd_hip.so"), str(tmp_path / "product"))
    assert set(got) == LAUNCHABLE, (sorted(set(got) - LAUNCHABLE), sorted(LAUNCHABLE - set(got)))
    for name, res in sorted(got.items()):
        assert res == (0, 0, 0), f"{name}: {res[0]} spilled VGPRs, {res[1]} spilled SGPRs, {res[2]} B of scratch"


def test_tuning_library_keeps_the_variants(tmp_path):
    tune = os.path.join(os.path.dirname(capi.__file__), "libpbd_hip_tune.so")
    assert os.path.exists(tune), "libpbd_hip_tune.so missing: `make -C partsbaseddetector_amd/csrc` builds it next to libpbd_hip.so"
    families = {n.split("<")[0].split("::")[-1] for n in _conv_kernels(tune, str(tmp_path / "tune"))}
    assert {"k_conv_glds", "k_conv_mfma", "k_conv_split32p"} <= families, sorted(families)
