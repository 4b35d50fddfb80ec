------------------------------ MODULE refuse_prime ------------------------------
(* Refused: a prime on something that is no variable name. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm refuse_prime
variables x = 0, y = 0;

process P \in 1..2
begin
  a: x := x + 1;
  b: y := y + x;
end process

end algorithm *)

Bad == (x + 1)' > x
=============================================================================
