/*
 * The `knn_vector` field (MapperPlugin.getMappers, S/plugins/MapperPlugin.java:59):
 *   {"type": "knn_vector", "dimension": 768, "data_type": "float" | "byte",
 *    "space_type": "l2" | "innerproduct" | "cosinesimil" | "dot_product", "method": {...}}
 *   {"type": "knn_vector", "dimension": 768, "data_type": "binary", "space_type": "hamming"}
 * indexed as Lucene's KnnFloatVectorField / KnnByteVectorField with the space type's VectorSimilarityFunction;
 * the codec (GpuKnnCodec) gives the field GpuFlatVectorsFormat.  A binary field holds packed bits: its dimension
 * counts bits (a multiple of 8, at most 8 x MAX_DIMS), a vector is dimension / 8 integers in [-128, 127], and
 * space_type is hamming (its default; no other pairs with binary, and hamming pairs with nothing else).  Lucene
 * can only record one of its own similarity ordinals, so the field is written as a byte field under EUCLIDEAN
 * with the field attribute BINARY_ATTRIBUTE, and GpuFlatVectorsReader stages it with OSK_HAMMING.  Python
 * mirror and contract tests: opensearch_amd/dsl.py, tests/test_dsl.py, tests/test_hamming_cpu.py.
 */
package org.opensearch.knn.gpu;

import java.io.IOException;
import java.util.ArrayList;
import java.util.Collections;
import java.util.List;
import java.util.Map;

import org.apache.lucene.document.FieldType;
import org.apache.lucene.document.KnnByteVectorField;
import org.apache.lucene.document.KnnFloatVectorField;
import org.apache.lucene.index.VectorEncoding;
import org.apache.lucene.index.VectorSimilarityFunction;
import org.apache.lucene.search.FieldExistsQuery;
import org.apache.lucene.search.Query;
import org.opensearch.core.xcontent.XContentParser;
import org.opensearch.index.mapper.MappedFieldType;
import org.opensearch.index.mapper.ParametrizedFieldMapper;
import org.opensearch.index.mapper.ParseContext;
import org.opensearch.index.mapper.SourceValueFetcher;
import org.opensearch.index.mapper.TextSearchInfo;
import org.opensearch.index.mapper.ValueFetcher;
import org.opensearch.index.query.QueryShardContext;
import org.opensearch.index.query.QueryShardException;
import org.opensearch.search.lookup.SearchLookup;

public final class KnnVectorFieldMapper extends ParametrizedFieldMapper {
    public static final String CONTENT_TYPE = "knn_vector";

    /** FieldInfo attribute of a binary (packed bits, Hamming) field: the reader stages it with OSK_HAMMING. */
    public static final String BINARY_ATTRIBUTE = "knn_vector.binary";

    static VectorSimilarityFunction similarity(String spaceType) {
        switch (spaceType) {
            case "hamming": return VectorSimilarityFunction.EUCLIDEAN;   // the ordinal Lucene records; see above
            case "l2": return VectorSimilarityFunction.EUCLIDEAN;
            case "innerproduct": return VectorSimilarityFunction.MAXIMUM_INNER_PRODUCT;
            case "cosinesimil": return VectorSimilarityFunction.COSINE;
            case "dot_product": return VectorSimilarityFunction.DOT_PRODUCT;
            default: throw new IllegalArgumentException("unknown space_type [" + spaceType + "]");
        }
    }

    private static KnnVectorFieldMapper toType(org.opensearch.index.mapper.FieldMapper in) {
        return (KnnVectorFieldMapper) in;
    }

    public static final class Builder extends ParametrizedFieldMapper.Builder {
        private final Parameter<Integer> dimension = Parameter.intParam("dimension", false, m -> toType(m).dimension, -1)
            .setValidator(d -> {
                // (binary: bits, up to 8 x MAX_DIMS; build() checks the range of the field's own data_type)
                if (d < 1 || d > 8 * GpuFlatVectorsFormat.MAX_DIMS)
                    throw new IllegalArgumentException("dimension must be in [1, " + GpuFlatVectorsFormat.MAX_DIMS
                        + "] (binary: a multiple of 8 in [8, " + 8 * GpuFlatVectorsFormat.MAX_DIMS + "]), got " + d);
            });
        private final Parameter<String> dataType = Parameter.restrictedStringParam("data_type", false,
            m -> toType(m).dataType, "float", "byte", "binary");
        private final Parameter<String> spaceType = Parameter.restrictedStringParam("space_type", false,
            m -> toType(m).spaceType, "l2", "innerproduct", "cosinesimil", "dot_product", "hamming");
        private final Parameter<Map<String, String>> meta = Parameter.metaParam();

        public Builder(String name) {
            super(name);
        }

        @Override
        protected List<Parameter<?>> getParameters() {
            return List.of(dimension, dataType, spaceType, meta);
        }

        /** space_type as written, or its default: hamming for a binary field, l2 otherwise. */
        String resolvedSpaceType() {
            boolean binary = "binary".equals(dataType.getValue());
            return spaceType.isConfigured() ? spaceType.getValue() : (binary ? "hamming" : "l2");
        }

        @Override
        public KnnVectorFieldMapper build(BuilderContext context) {
            boolean binary = "binary".equals(dataType.getValue());
            String space = resolvedSpaceType();
            int d = dimension.getValue();
            if (binary != "hamming".equals(space))
                throw new IllegalArgumentException("[space_type] hamming and [data_type] binary go together only: got "
                    + "[space_type] " + space + " with [data_type] " + dataType.getValue());
            if (binary ? (d < 8 || d % 8 != 0) : d > GpuFlatVectorsFormat.MAX_DIMS)
                throw new IllegalArgumentException(binary
                    ? "dimension of a [data_type] binary field must be a multiple of 8 in [8, "
                        + 8 * GpuFlatVectorsFormat.MAX_DIMS + "], got " + d
                    : "dimension must be in [1, " + GpuFlatVectorsFormat.MAX_DIMS + "], got " + d);
            KnnVectorFieldType ft = new KnnVectorFieldType(buildFullName(context), d,
                "float".equals(dataType.getValue()) ? VectorEncoding.FLOAT32 : VectorEncoding.BYTE,
                similarity(space), binary, meta.getValue());
            return new KnnVectorFieldMapper(name, ft, multiFieldsBuilder.build(this, context), copyTo.build(), this);
        }
    }

    public static final TypeParser PARSER = new TypeParser((n, c) -> new Builder(n));

    /** The field type: its dimension, encoding and similarity decide the Lucene field and the query. */
    public static final class KnnVectorFieldType extends MappedFieldType {
        private final int dimension;
        private final VectorEncoding encoding;
        private final VectorSimilarityFunction similarity;
        private final boolean binary;

        public KnnVectorFieldType(String name, int dimension, VectorEncoding encoding, VectorSimilarityFunction similarity,
                                  boolean binary, Map<String, String> meta) {
            super(name, false, false, false, TextSearchInfo.NONE, meta);
            this.dimension = dimension;
            this.encoding = encoding;
            this.similarity = similarity;
            this.binary = binary;
        }

        public int dimension() {
            return dimension;
        }

        /** Packed bits under Hamming distance (data_type binary): dimension counts bits. */
        public boolean isBinary() {
            return binary;
        }

        /** Elements of a document / query vector, the Lucene field's dimension: dimension, or (binary) dimension / 8. */
        public int vectorLength() {
            return binary ? dimension / 8 : dimension;
        }

        public boolean isByte() {
            return encoding == VectorEncoding.BYTE;
        }

        public VectorSimilarityFunction similarity() {
            return similarity;
        }

        /** A query vector as bytes for a byte field: every component an integer in [-128, 127]. */
        public byte[] toBytes(float[] v) {
            byte[] b = new byte[v.length];
            for (int i = 0; i < v.length; i++) {
                if (v[i] != Math.rint(v[i]) || v[i] < -128 || v[i] > 127)
                    throw new IllegalArgumentException("byte vector component [" + v[i] + "] is not an integer in [-128, 127]");
                b[i] = (byte) v[i];
            }
            return b;
        }

        @Override
        public String typeName() {
            return CONTENT_TYPE;
        }

        @Override
        public ValueFetcher valueFetcher(QueryShardContext context, SearchLookup searchLookup, String format) {
            return SourceValueFetcher.identity(name(), context, format);
        }

        @Override
        public Query existsQuery(QueryShardContext context) {
            return new FieldExistsQuery(name());
        }

        @Override
        public Query termQuery(Object value, QueryShardContext context) {
            throw new QueryShardException(context, "knn_vector field [" + name() + "] supports only the knn query");
        }
    }

    private final int dimension;
    private final String dataType, spaceType;

    private KnnVectorFieldMapper(String simpleName, KnnVectorFieldType ft, MultiFields multiFields, CopyTo copyTo, Builder b) {
        super(simpleName, ft, multiFields, copyTo);
        this.dimension = b.dimension.getValue();
        this.dataType = b.dataType.getValue();
        this.spaceType = b.resolvedSpaceType();
    }

    @Override
    public KnnVectorFieldType fieldType() {
        return (KnnVectorFieldType) super.fieldType();
    }

    @Override
    protected void parseCreateField(ParseContext context) throws IOException {
        XContentParser parser = context.parser();
        List<Float> values = new ArrayList<>();
        if (parser.currentToken() != XContentParser.Token.START_ARRAY)
            throw new IllegalArgumentException("knn_vector field [" + name() + "] expects an array of numbers");
        for (XContentParser.Token t = parser.nextToken(); t != XContentParser.Token.END_ARRAY; t = parser.nextToken())
            values.add(parser.floatValue());
        KnnVectorFieldType ft = fieldType();
        if (values.size() != ft.vectorLength())
            throw new IllegalArgumentException("vector of field [" + name() + "] has " + values.size() + " dims, the mapping "
                + ft.vectorLength());
        float[] v = new float[values.size()];
        for (int i = 0; i < v.length; i++) v[i] = values.get(i);
        if (ft.isBinary()) {
            FieldType binaryType = new FieldType();
            binaryType.setVectorAttributes(v.length, VectorEncoding.BYTE, ft.similarity());
            binaryType.putAttribute(BINARY_ATTRIBUTE, "true");
            binaryType.freeze();
            context.doc().add(new KnnByteVectorField(ft.name(), ft.toBytes(v), binaryType));
        } else if (ft.isByte()) {
            context.doc().add(new KnnByteVectorField(ft.name(), ft.toBytes(v), ft.similarity()));
        } else {
            context.doc().add(new KnnFloatVectorField(ft.name(), v, ft.similarity()));
        }
    }

    @Override
    public ParametrizedFieldMapper.Builder getMergeBuilder() {
        return new Builder(simpleName()).init(this);
    }

    @Override
    protected String contentType() {
        return CONTENT_TYPE;
    }
}
