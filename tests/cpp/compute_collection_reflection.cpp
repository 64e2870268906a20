// compute_collection_reflection.cpp — host only: what szg::ComputeCollectionPipeline (include/szg/pipelines.hpp) reports about
// its four programs, printed as one JSON document, and a walk over its accessors. No device is touched: the constructor reads
// the library's tables. tests/test_compute_collection_reflection.py compiles it and compares the output with the reflection of
// the reference's binaries (tests/golden/compute_collection_reflection.json).
#include <cstdio>
#include <cstring>

#include "szg/pipelines.hpp"

int main()
{
    szg::ComputeCollectionPipeline collection;
    std::printf("{\"valid\": %d, \"count\": %zu, \"index\": %zu, \"shaders\": [", collection.valid() ? 1 : 0, collection.shaderCount(),
                collection.shaderIndex());
    size_t program = 0;
    for (szg::ComputeCollectionPipeline::PushConstant const& r : collection.shaders())
    {
        collection.selectShader(program);
        bool zeros = true;
        for (uint8_t b : collection.readPushConstantBytes())
        {
            zeros = zeros && b == 0;
        }
        bool const same = std::strcmp(collection.currentShader().name, r.name) == 0 && collection.shaderIndex() == program;
        std::printf("%s{\"name\": \"%s\", \"size\": %u, \"padded_size\": %u, \"layout_offset\": %u, \"local_size\": [%u, %u, %u], "
                    "\"block_bytes\": %zu, \"zeros\": %d, \"current_is_selected\": %d, \"members\": [",
                    program ? ", " : "", r.name, r.size_bytes, r.padded_size_bytes, r.layout_offset_bytes, r.local_size[0], r.local_size[1],
                    r.local_size[2], collection.mapPushConstantBytes().size(), zeros ? 1 : 0, same ? 1 : 0);
        for (uint32_t i = 0; i < r.member_count; i++)
        {
            szg_cc_member const& m = r.members[i];
            std::printf("%s{\"name\": \"%s\", \"offset\": %u, \"size\": %u, \"padded_size\": %u, \"component_type\": %u, \"vector_width\": %u, "
                        "\"column_count\": %u}",
                        i ? ", " : "", m.name, m.offset_bytes, m.size_bytes, m.padded_size_bytes, m.component_type, m.vector_width,
                        m.column_count);
        }
        std::printf("]}");
        program++;
    }
    // a block keeps its bytes while another program is selected; an index outside the table changes nothing
    collection.selectShader(1);
    float const bottom[4] = {1.0f, 0.5f, 0.25f, 1.0f};
    bool const wrote = collection.writePushConstant<float>("bottomColor", bottom);
    collection.selectShader(3);
    collection.selectShader(7);
    size_t const after = collection.shaderIndex();
    collection.selectShader(1);
    bool const kept = std::memcmp(collection.readPushConstantBytes().data() + 32, bottom, sizeof bottom) == 0;
    std::printf("], \"wrote\": %d, \"index_after_7\": %zu, \"kept\": %d}\n", wrote ? 1 : 0, after, kept ? 1 : 0);
    return 0;
}
