/*
 * The parties' responses consumed as they arrive (include/amphora_client_session.h): each
 * worker of AmphoraCommunicationClient's parallelStream (AmphoraCommunicationClient.java:150-154)
 * hands the five base64 strings of its party's VerifiableSecretShare / OutputDeliveryObject body
 * to addTexts the moment the party has answered -- one launch decodes them on the GPU and adds
 * them into five running sums -- and secrets / maskedRecords / maskedDataText finish from the
 * sums alone: the values and exceptions of getSecret (DefaultAmphoraClient.java:206-217) and
 * createSecret (:150-170) on all the bodies.  All but the last response are uploaded and decoded
 * while the client still waits for the slowest party.
 *
 * Any thread may hand in its own party; finish and close belong to one thread, after the
 * addTexts calls have returned.  A session finishes once.
 *
 * Unbuildable in this image (no JDK): compiled by jni/Makefile against the
 * reference's classpath when one is present.
 */
package io.carbynestack.amphora.client;

import static io.carbynestack.amphora.client.NativeShareArithmetic.WORD_WIDTH;

import io.carbynestack.amphora.common.exceptions.IntegrityVerificationException;
import java.math.BigInteger;
import java.nio.charset.StandardCharsets;
import java.util.ArrayList;
import java.util.List;

class ResponseSession implements AutoCloseable {
  private final SecretShareUtil util;
  private final int parties;
  private long session;
  private int words = -1;

  ResponseSession(SecretShareUtil util, int parties) {
    this.util = util;
    this.parties = parties;
  }

  /** 16-byte words of a base64 field text (Jackson's MIME_NO_LINEFEEDS: '=' padding, no breaks) */
  static int wordsOfBase64(String text) {
    int n = text.length();
    int pad = n >= 2 ? (text.charAt(n - 1) == '=' ? 1 : 0) + (text.charAt(n - 2) == '=' ? 1 : 0) : 0;
    int bytes = n / 4 * 3 - pad;
    if (n % 4 != 0 || bytes % WORD_WIDTH != 0) {
      throw new IllegalArgumentException("base64 field is not a whole number of words");
    }
    return bytes / WORD_WIDTH;
  }

  /**
   * One party's five base64 strings, parties in any order, each once. The first call fixes the
   * word count.
   *
   * @throws IllegalArgumentException for fields of unequal length, another length than the first
   *     party's, or an illegal base64 character (reported again, the smallest over all parties,
   *     by the finish call)
   */
  void addTexts(
      int party, String secretShares, String rShares, String vShares, String wShares, String uShares) {
    synchronized (this) {
      if (session == 0) {
        words = wordsOfBase64(secretShares);
        session = NativeShareArithmetic.clientBegin(util.nativeContext(), words, parties);
      }
    }
    NativeShareArithmetic.clientParty(
        session,
        party,
        secretShares.getBytes(StandardCharsets.US_ASCII),
        rShares.getBytes(StandardCharsets.US_ASCII),
        vShares.getBytes(StandardCharsets.US_ASCII),
        wShares.getBytes(StandardCharsets.US_ASCII),
        uShares.getBytes(StandardCharsets.US_ASCII));
  }

  /**
   * getSecret's arithmetic from the sums: the canonical secrets.
   *
   * @throws IntegrityVerificationException for the smallest failing word, with the reference's
   *     message
   */
  List<BigInteger> secrets() {
    byte[] out = new byte[words * WORD_WIDTH];
    long fail = NativeShareArithmetic.clientFinishVerify(handle(), out);
    if (fail >= 0) {
      throw failureAt(fail);
    }
    return NativeShareArithmetic.unpack(out, words);
  }

  /**
   * createSecret's arithmetic from the sums: the 24-character base64 record of every masked word.
   *
   * @throws IntegrityVerificationException for the smallest failing mask word
   * @throws IndexOutOfBoundsException if the secret has more words than masks (after the masks
   *     verified, as inputMasks.get(i) fails in the reference)
   */
  List<String> maskedRecords(BigInteger[] secret) {
    moreSecretsThanMasks(secret.length);
    byte[] rec = new byte[24 * secret.length];
    long fail =
        NativeShareArithmetic.clientFinishMask(
            handle(), NativeShareArithmetic.pack(secret, secret.length, util.getPrime()), rec);
    if (fail >= 0) {
      throw failureAt(fail);
    }
    List<String> out = new ArrayList<>(secret.length);
    for (int i = 0; i < secret.length; i++) {
      out.add(new String(rec, 24 * i, 24, StandardCharsets.US_ASCII));
    }
    return out;
  }

  /** maskedRecords framed as the "data" array text of the MaskedInput body */
  String maskedDataText(BigInteger[] secret) {
    moreSecretsThanMasks(secret.length);
    byte[] text = new byte[secret.length == 0 ? 2 : 37 * secret.length + 1];
    long fail =
        NativeShareArithmetic.clientFinishMaskJson(
            handle(), NativeShareArithmetic.pack(secret, secret.length, util.getPrime()), text);
    if (fail >= 0) {
      throw failureAt(fail);
    }
    return new String(text, StandardCharsets.US_ASCII);
  }

  @Override
  public synchronized void close() {
    if (session != 0) {
      NativeShareArithmetic.clientFree(session);
      session = 0;
    }
  }

  private synchronized long handle() {
    if (session == 0) {
      throw new IllegalStateException("no response was added");
    }
    return session;
  }

  // more secret words than masks: every mask is verified first (a finish with no secrets),
  // then inputMasks.get(i) fails (DefaultAmphoraClient.java:153 before :155-157)
  private void moreSecretsThanMasks(int secretWords) {
    if (secretWords <= words) {
      return;
    }
    long fail = NativeShareArithmetic.clientFinishMask(handle(), new byte[0], new byte[0]);
    if (fail >= 0) {
      throw failureAt(fail);
    }
    throw new IndexOutOfBoundsException("Index " + words + " out of bounds for length " + words);
  }

  // the reference's message from the five sums of the failing word: y, r, v, w, u
  private IntegrityVerificationException failureAt(long word) {
    byte[] w = NativeShareArithmetic.clientWord(session, word);
    BigInteger[] x = new BigInteger[5];
    for (int k = 0; k < 5; k++) x[k] = NativeShareArithmetic.word(w, k);
    return new IntegrityVerificationException(util.failureMessage(x[0], x[1], x[4], x[2], x[3]));
  }
}
