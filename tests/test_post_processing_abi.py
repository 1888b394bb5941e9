"""CPU tests of the post-processing boundary: the entry points of include/ptamd.h are exported and bound, the two structs have the layout
the numpy / ctypes mirrors assume (checked by a gcc-compiled probe), the C++ mirror compiles on its own, and pt_demo's PNG writer
produces files PIL decodes to the same pixels."""
import ctypes as C
import os
import subprocess

import numpy as np

import __graft_entry__ as ge

NEW = ["pt_post_set_constants", "pt_post_render", "pt_post_download_bloom"]


def test_post_entry_points_are_declared_exported_and_bound(ptamd):
    header = open(os.path.join(ge.ROOT, "include", "ptamd.h")).read()
    lib = ptamd.load_library()
    for name in NEW:
        assert f"int {name}(" in header
        assert hasattr(lib, name) and name in ptamd.EXPORTS
        assert getattr(lib, name).argtypes is not None


def test_struct_layouts_match_a_compiled_probe(tmp_path, pkg, ptamd):
    L = pkg.layouts
    fields = ["RenderSize", "IsBloomEnabled", "BloomStrength", "IsHDREnabled", "ToneMappingOperator", "Exposure", "PaperWhiteNits",
              "ColorPrimaryRotation", "_pad"]
    tex = ["Radiance", "Color", "BackBuffer", "Display8"]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "include/ptamd.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(PtPostProcessSettings), sizeof(PtPostTextures));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(PtPostProcessSettings, {f}));\n' for f in fields)
                   + "".join(f'  printf("%zu\\n", offsetof(PtPostTextures, {f}));\n' for f in tex)
                   + f'  printf("%d %d %d %d %d %d\\n", PT_TONE_MAP_SATURATE, PT_TONE_MAP_REINHARD, PT_TONE_MAP_ACES_FILMIC,'
                     f' PT_COLOR_ROTATION_HDTV_TO_UHDTV, PT_COLOR_ROTATION_DCI_P3_D65_TO_UHDTV, PT_COLOR_ROTATION_HDTV_TO_DCI_P3_D65);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", ge.ROOT, str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    size_s, size_t = (int(v) for v in out[0].split())
    assert size_s == L.POST_PROCESS_SETTINGS.itemsize == 48
    assert size_t == C.sizeof(ptamd.PostTextures) == 32
    offs = [int(v) for v in out[1:1 + len(fields)]]
    assert offs[:-1] == [L.POST_PROCESS_SETTINGS.fields[f][1] for f in fields[:-1]] and offs[-1] == 36
    assert [int(v) for v in out[1 + len(fields):1 + len(fields) + len(tex)]] == [getattr(ptamd.PostTextures, f).offset for f in tex]
    enums = [int(v) for v in out[1 + len(fields) + len(tex)].split()]
    assert enums == [L.TONE_MAP_SATURATE, L.TONE_MAP_REINHARD, L.TONE_MAP_ACES_FILMIC, L.COLOR_ROTATION_HDTV_TO_UHDTV,
                     L.COLOR_ROTATION_DCI_P3_D65_TO_UHDTV, L.COLOR_ROTATION_HDTV_TO_DCI_P3_D65]


def test_cpp_mirror_header_compiles_standalone_with_post_processing(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "directx-physically-based-raytracer_amd/host/ptamd.hpp"\n'
                   'int main() { ptamd::PostProcessing::Settings s; s.ToneMapping.HDR.PaperWhiteNits = 400;\n'
                   '  s.ToneMapping.NonHDR.Operator = ptamd::PostProcessing::ToneMapOperator::Reinhard;\n'
                   '  s.ToneMapping.HDR.ColorPrimaryRotation = ptamd::PostProcessing::ColorRotation::DCI_P3_D65toUHDTV;\n'
                   '  return (int)s.Bloom.IsEnabled + (int)s.ToneMapping.NonHDR.Exposure; }\n')
    subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Werror", "-fsyntax-only", "-I", ge.ROOT, str(src)])


def test_png_writer_round_trips_through_pil(tmp_path):
    from PIL import Image
    drv = tmp_path / "png.cpp"
    drv.write_text('#include "directx-physically-based-raytracer_amd/host/pt_png.hpp"\n#include <cstdlib>\n'
                   'int main(int argc, char** argv) {\n'
                   '  const uint32_t w = (uint32_t)atoi(argv[2]), h = (uint32_t)atoi(argv[3]);\n'
                   '  std::vector<uint8_t> rgba((size_t)w * h * 4);\n'
                   '  FILE* fp = fopen(argv[1], "rb"); if (!fp || fread(rgba.data(), 1, rgba.size(), fp) != rgba.size()) return 2; fclose(fp);\n'
                   '  return ptpng::write_rgb(argv[4], rgba.data(), w, h) ? 0 : 1; }\n')
    exe = tmp_path / "png"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ge.ROOT, str(drv), "-o", str(exe)])
    rng = np.random.default_rng(7)
    for w, h in ((1, 1), (37, 5), (300, 250)):              # 300 x 250 x 3 + rows > 65535: several stored blocks
        rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        raw, png = tmp_path / f"{w}x{h}.rgba", tmp_path / f"{w}x{h}.png"
        rgba.tofile(raw)
        subprocess.check_call([str(exe), str(raw), str(w), str(h), str(png)])
        im = Image.open(png)
        im.load()                                            # checks every CRC and the Adler-32 of the zlib stream
        assert im.mode == "RGB" and im.size == (w, h)
        assert np.array_equal(np.asarray(im), rgba[..., :3])
